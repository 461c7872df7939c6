"""Centrelines' semantics (include/infur_hip.h) applied literally: a sequential tracer over the links of the kept pixels, in plain
numpy and Python.  Slow and plain on purpose; the device is compared with it by ``==``."""
import numpy as np

import skeleton_ref as S

OFFSET, COUNT, VALUE, A, B, ORTHO, DIAG, MIN_H, WORDS = range(9)
BRANCHES, VERTICES, LINKS, NODES, ENDS, RINGS, C_DIAG, STATUS, COUNT_WORDS = range(9)
SKIP, CORNERS = 1, 2
OVERFLOW = 1


def links(plane, kind=None, skip=None):
    """-> (kept [h, w] bool, link [8, h, w] bool): every set 4-neighbour, and a set diagonal neighbour when neither of the two common
    4-neighbours is set"""
    kept = np.ones(plane.shape, bool) if skip is None else plane != skip
    if kind is not None:
        kept &= np.asarray(kind) != 0
    P = S.neighbours(plane, kept)
    link = P.copy()
    for k in (1, 3, 5, 7):
        link[k] = P[k] & ~P[k - 1] & ~P[(k + 1) & 7]
    return kept, link


def centrelines(plane, kind=None, height=None, skip=None, corners=False, max_links=0):
    """-> (records [branches, 8] u32, vertices [n] u32, counts [8] u32)"""
    plane = np.asarray(plane)
    h, w = plane.shape
    counts = np.zeros(COUNT_WORDS, np.uint32)
    none = np.zeros((0, WORDS), np.uint32), np.zeros(0, np.uint32), counts
    if plane.size == 0:
        return none
    kept, link = links(plane, kind, skip)
    d = link.sum(0)
    counts[[LINKS, NODES, ENDS, C_DIAG]] = d.sum() // 2, (kept & (d != 2)).sum(), (kept & (d == 1)).sum(), link[1::2].sum() // 2
    if counts[LINKS] > (max_links if max_links else 2 * h * w):
        counts[STATUS] = OVERFLOW
        return none
    step = [dy * w + dx for dy, dx in S.DIRS]
    flat = link.reshape(8, -1)
    dirs = {int(p): [k for k in range(8) if flat[k, p]] for p in np.flatnonzero(kept.ravel())}
    hgt = (lambda p: int(height.flat[p])) if height is not None else (lambda p: 0)

    def walk(p, k):
        """from pixel p along direction k to the next node, or back to p on a ring -> (pixels, directions)"""
        px, ks = [p], []
        while True:
            ks.append(k)
            p += step[k]
            px.append(p)
            if len(dirs[p]) != 2 or p == px[0]:
                return px, ks
            k = [j for j in dirs[p] if j != k ^ 4][0]

    found, seen = [], set()  # (first dart, pixels, directions, closed); the ring pixels already listed
    for p in sorted(dirs):
        if not dirs[p]:
            found.append((8 * p, [p], [], False))
        elif len(dirs[p]) != 2:
            for k in dirs[p]:
                px, ks = walk(p, k)
                if 8 * p + k < 8 * px[-1] + (ks[-1] ^ 4):  # the smaller of the branch's two first darts
                    found.append((8 * p + k, px, ks, False))
    for p in sorted(dirs):  # what is left of the path pixels lies on rings
        if len(dirs[p]) == 2 and p not in seen:
            px, ks = walk(p, dirs[p][0])
            if len(dirs[px[-1]]) == 2:  # it came back: p is the ring's smallest pixel
                found.append((8 * p + ks[0], px, ks, True))
                seen.update(px)
                counts[RINGS] += 1
            else:  # a branch between nodes, listed above
                seen.update(px[:-1] + walk(p, dirs[p][1])[0][:-1])
    records, vertices = [], []
    for _, px, ks, closed in sorted(found):
        keep = [i for i in range(len(px)) if not corners or i in (0, len(px) - 1) or ks[i - 1] != ks[i]]
        ndiag = sum(k & 1 for k in ks)
        records.append((len(vertices), len(keep), int(plane.flat[px[0]]), px[0], px[-1], len(ks) - ndiag, ndiag, min(hgt(p) for p in px)))
        vertices += [px[i] for i in keep]
    counts[BRANCHES], counts[VERTICES] = len(records), len(vertices)
    return np.array(records, np.uint32).reshape(-1, WORDS), np.array(vertices, np.uint32), counts
