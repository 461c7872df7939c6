"""Skeleton's semantics (include/infur_hip.h) applied literally in numpy: Guo and Hall's two-sub-iteration thinning of every value as
its own binary mask, then the measures.  Slow and plain on purpose; the device is compared with it by ``==``."""
import numpy as np

PIXELS, ENDS, JUNCTIONS, ORTHO, DIAG, FIRST, MIN_H, MAX_H, WORDS = range(9)
KEPT, REMOVED, ROUNDS, C_ENDS, C_JUNCTIONS, C_ORTHO, C_DIAG, STATUS, COUNT_WORDS = range(9)
UNFINISHED = 1
NONE = 0xFFFFFFFF
# P2 .. P9 = N, NE, E, SE, S, SW, W, NW as (dy, dx)
DIRS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def neighbours(plane, alive):
    """-> [8, h, w] bool: neighbour k of p is inside the frame, alive and holds p's value"""
    h, w = plane.shape
    val = np.full((h + 2, w + 2), -1, np.int64)
    val[1:-1, 1:-1] = np.where(alive, plane.astype(np.int64), -1)
    return np.stack([val[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] == np.where(alive, plane.astype(np.int64), -2) for dy, dx in DIRS])


def dies(plane, alive, k):
    """the alive pixels sub-iteration k (1-based) removes"""
    P2, P3, P4, P5, P6, P7, P8, P9 = neighbours(plane, alive)
    i = lambda b: b.astype(np.int64)  # noqa: E731
    C = i(~P2 & (P3 | P4)) + i(~P4 & (P5 | P6)) + i(~P6 & (P7 | P8)) + i(~P8 & (P9 | P2))
    N = np.minimum(i(P9 | P2) + i(P3 | P4) + i(P5 | P6) + i(P7 | P8), i(P2 | P3) + i(P4 | P5) + i(P6 | P7) + i(P8 | P9))
    m = ((P6 | P7 | ~P9) & P8) if k % 2 == 1 else ((P2 | P3 | ~P5) & P4)
    return alive & (C == 1) & (N >= 2) & (N <= 3) & ~m


def thin(plane, skip=None, max_rounds=0):
    """-> (alive after the last sub-iteration, ROUNDS, the effective max_rounds)"""
    alive = np.ones(plane.shape, bool) if skip is None else plane != skip
    limit = max_rounds if max_rounds else min(plane.shape) + 2
    rounds = quiet = 0
    for k in range(1, limit + 1):
        d = dies(plane, alive, k)
        alive = alive & ~d
        rounds, quiet = (k, 0) if d.any() else (rounds, quiet + 1)
        if quiet == 2:
            break
    return alive, rounds, limit


def skeleton(plane, height=None, skip=None, max_rounds=0, rows=None):
    """-> (kind [h, w] u8, table [rows, 8] u32, counts [8] u32)"""
    plane = np.asarray(plane)
    rows = (int(plane.max()) + 1 if plane.size else 0) if rows is None else rows
    table = np.zeros((rows, WORDS), np.uint32)
    table[:, FIRST] = NONE
    if plane.size == 0:
        return np.zeros(plane.shape, np.uint8), table, np.zeros(COUNT_WORDS, np.uint32)
    start = np.ones(plane.shape, bool) if skip is None else plane != skip
    alive, rounds, limit = thin(plane, skip, max_rounds)
    P = neighbours(plane, alive)
    P2, P3, P4, P5, P6, P7, P8, P9 = P
    n = P.sum(0)
    kind = np.where(alive, 1 + n, 0).astype(np.uint8)
    # every pair at its pixel of smaller index: E and S; SE and SW when neither common 4-neighbour is a kept pixel of the value
    ortho = alive * (P4.astype(np.int64) + P6)
    diag = alive * ((P5 & ~P4 & ~P6).astype(np.int64) + (P7 & ~P8 & ~P6))
    ends, junctions = alive & (n == 1), alive & (n >= 3)
    index = np.arange(plane.size).reshape(plane.shape)
    for v in np.unique(plane[alive]):
        if v >= rows:
            continue
        sel = alive & (plane == v)
        hs = height[sel] if height is not None else np.zeros(1, np.uint32)
        table[v] = (sel.sum(), ends[sel].sum(), junctions[sel].sum(), ortho[sel].sum(), diag[sel].sum(), index[sel].min(), hs.min(), hs.max())
    counts = np.array([alive.sum(), start.sum() - alive.sum(), rounds, ends.sum(), junctions.sum(), ortho.sum(), diag.sum(),
                       UNFINISHED if limit < rounds + 2 else 0], np.uint32)
    return kind, table, counts


def plus(h, w, arm=5):
    """a plus sign of value 1 on 0 whose arms, `arm` pixels thick, run from edge to edge through the centre"""
    p = np.zeros((h, w), np.uint8)
    p[h // 2 - arm // 2:h // 2 - arm // 2 + arm, :] = 1
    p[:, w // 2 - arm // 2:w // 2 - arm // 2 + arm] = 1
    return p
