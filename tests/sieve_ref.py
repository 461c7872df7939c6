"""Reference of Adjacency and Sieve for the tests: numpy only, no product code, built on ``regions_ref.label``.

Semantics (include/infur_hip.h), applied literally:

* Adjacency.  A pixel is *inside* when its value is below ``rows`` and is not ``skip_value`` (flag ``SKIP``).  A *border edge* is a
  pixel edge between two 4-neighbours that are both inside and differ.  The edge between (x, y) and (x+1, y) has id 2 (y w + x),
  the edge between (x, y) and (x, y+1) id 2 (y w + x) + 1.  One record (A, B, BORDER, FIRST) per unordered pair with A < B, in
  ascending FIRST (the pair's smallest edge id); per value (DEGREE, LONGEST, BORDER, PERIMETER), LONGEST the neighbour with the
  longest border, ties to the smallest value, PERIMETER every pixel edge of the value against anything else, the frame included;
  counts = PAIRS, EDGES, SKIPPED, OUTSIDE, RUNS, WRITTEN, 0, STATUS.
* RUNS = R: the maximal sequences of border edges between rows y and y+1 that are consecutive in x and have the same ordered (top,
  bottom) pair, plus those between columns x and x+1, consecutive in y, with the same ordered (left, right) pair.
  ``2 R > pair_slots`` (0: 2^20) is ``OVERFLOW``: no record, rows (0, NONE, 0, PERIMETER), PAIRS = EDGES = WRITTEN = 0.
  ``TRUNCATED``: records are wanted and PAIRS > pair_rows.
* Sieve, on what Regions gives with min_pixels = 0 and no skip: n = min(n_regions, table_rows); a pixel whose label is >= n is
  fixed; region r is small when PIXELS(r) < min_pixels; round 0 resolves the kept regions with their own class; in round t >= 1
  every unresolved region takes, among the neighbours resolved after round t-1, the one with the largest BORDER (ties to the
  smallest id) and with it its class and its INTO; the loop ends after the first round that resolves nothing or after max_rounds
  (0: 8) rounds; what is left is stranded.  rows = (CLASS, INTO, ROUND, BORDER), counts = REGIONS, SMALL, ABSORBED, STRANDED,
  ROUNDS, PIXELS_CHANGED, PAIRS, STATUS.

``adjacency`` and ``sieve`` are vectorised; ``brute_adjacency`` and ``brute_sieve`` are plain double loops over pixels, edges,
regions and pairs, with R counted from its definition.
"""
import numpy as np

import regions_ref as R

NONE = 0xFFFFFFFF
SKIP = 1
A, B, BORDER, FIRST, PAIR_WORDS = range(5)
DEGREE, LONGEST, ROW_BORDER, PERIMETER, ROW_WORDS = range(5)
PAIRS, EDGES, SKIPPED, OUTSIDE, RUNS, WRITTEN, RESERVED, STATUS, COUNT_WORDS = range(9)
OVERFLOW, TRUNCATED = 1, 2
S_CLASS, S_INTO, S_ROUND, S_BORDER, SIEVE_ROW_WORDS = range(5)
S_REGIONS, S_SMALL, S_ABSORBED, S_STRANDED, S_ROUNDS, S_PIXELS_CHANGED, S_PAIRS, S_STATUS, SIEVE_COUNT_WORDS = range(9)
S_OVERFLOW, S_ROUNDS_EXHAUSTED, S_TABLE_SHORT = 1, 2, 4
DEFAULT_SLOTS, DEFAULT_ROUNDS, MAX_ROUNDS = 1 << 20, 8, 64

# the header's worked example: two speckles in a plane of two classes, one of which needs two rounds
WORKED = np.array([[1, 1, 1, 2, 2, 2],
                   [1, 3, 1, 2, 2, 2],
                   [1, 1, 1, 2, 4, 4],
                   [1, 1, 1, 2, 4, 5]], np.uint8)


class Adj:
    """pairs [min(PAIRS, pair_rows), 4] u32, rows [rows, 4] u32, counts [8] u32"""

    def __init__(self, pairs, rows, counts):
        self.pairs, self.rows, self.counts = pairs, rows, counts
        for arr in (pairs, rows, counts):
            arr.setflags(write=False)


class Sieved:
    """klass_out [h, w] u8, rows [n, 4] u32, counts [8] u32"""

    def __init__(self, klass_out, rows, counts):
        self.klass_out, self.rows, self.counts = klass_out, rows, counts
        for arr in (klass_out, rows, counts):
            arr.setflags(write=False)


def _inside(plane, rows, flags, skip_value):
    v = np.asarray(plane).astype(np.int64)
    assert v.ndim == 2
    skipped = (v == skip_value) if flags & SKIP else np.zeros(v.shape, bool)
    inside = ~skipped & (v < rows)
    return v, skipped, inside


def _finish(pair_list, perim, rows, runs, skipped, outside, pair_rows, pair_slots, want_pairs):
    """pair_list: [(a, b, border, first)] in any order"""
    slots = pair_slots or DEFAULT_SLOTS
    assert slots >= 64 and slots & (slots - 1) == 0
    over = 2 * runs > slots
    if over:
        pair_list = []
    pair_list = sorted(pair_list, key=lambda p: p[3])
    table = np.zeros((rows, ROW_WORDS), np.uint32)
    table[:, LONGEST] = NONE
    table[:, PERIMETER] = perim
    best = {}
    for a, b, n, _ in pair_list:
        for me, other in ((a, b), (b, a)):
            table[me, DEGREE] += 1
            if me not in best or (n, -other) > (best[me][0], -best[me][1]):
                best[me] = (n, other)
    for me, (n, other) in best.items():
        table[me, LONGEST], table[me, ROW_BORDER] = other, n
    n_pairs = len(pair_list)
    if pair_rows is None:
        pair_rows = n_pairs
    written = min(n_pairs, pair_rows) if want_pairs else 0
    counts = np.zeros(COUNT_WORDS, np.uint32)
    counts[PAIRS], counts[EDGES] = n_pairs, sum(p[2] for p in pair_list)
    counts[SKIPPED], counts[OUTSIDE], counts[RUNS], counts[WRITTEN] = skipped, outside, runs, written
    counts[STATUS] = (OVERFLOW if over else 0) | (TRUNCATED if want_pairs and n_pairs > pair_rows else 0)
    pairs = np.array(pair_list[:written], np.uint32).reshape(-1, PAIR_WORDS)
    return Adj(pairs, table, counts)


def adjacency(plane, rows, flags=0, skip_value=0, pair_rows=None, pair_slots=0, want_pairs=True):
    """pair_rows None: as many as there are"""
    v, skipped, inside = _inside(plane, rows, flags, skip_value)
    h, w = v.shape
    vi = np.where(inside, v, -1)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    # the edges to the right and the edges downwards
    la, lb, lid = vi[:, :-1], vi[:, 1:], 2 * idx[:, :-1]
    ta, tb, tid = vi[:-1], vi[1:], 2 * idx[:-1] + 1
    bh = (la >= 0) & (lb >= 0) & (la != lb)
    bv = (ta >= 0) & (tb >= 0) & (ta != tb)
    # R: a head is a border edge whose ordered pair differs from the pair one row up (right edges) or one column to the left
    head_h = bh.copy()
    head_h[1:] &= ~(bh[:-1] & (la[1:] == la[:-1]) & (lb[1:] == lb[:-1]))
    head_v = bv.copy()
    head_v[:, 1:] &= ~(bv[:, :-1] & (ta[:, 1:] == ta[:, :-1]) & (tb[:, 1:] == tb[:, :-1]))
    runs = int(head_h.sum()) + int(head_v.sum())
    a = np.concatenate([la[bh], ta[bv]])
    b = np.concatenate([lb[bh], tb[bv]])
    eid = np.concatenate([lid[bh], tid[bv]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.argsort(eid, kind="stable")
    key = (lo[order] << 32) | hi[order]
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    pair_list = [(int(k >> 32), int(k & 0xFFFFFFFF), int(n), int(eid[order][f])) for k, f, n in zip(uniq, first, count)]
    # PERIMETER: the sides of every inside pixel that face anything but its value
    pad = np.full((h + 2, w + 2), -2, np.int64)
    pad[1:-1, 1:-1] = np.where(inside, v, -1)
    sides = sum((pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] != vi).astype(np.int64) for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)))
    perim = np.bincount(v[inside], weights=sides[inside], minlength=rows)[:rows].astype(np.uint32) if rows else np.zeros(0, np.uint32)
    return _finish(pair_list, perim, rows, runs, int(skipped.sum()), int((~skipped & ~inside).sum()), pair_rows, pair_slots, want_pairs)


def brute_adjacency(plane, rows, flags=0, skip_value=0, pair_rows=None, pair_slots=0, want_pairs=True):
    plane = np.asarray(plane)
    h, w = plane.shape

    def val(y, x):  # the value of an inside pixel, else None
        u = int(plane[y, x])
        return None if (flags & SKIP and u == skip_value) or u >= rows else u

    def border(p, q):
        return p is not None and q is not None and p != q

    edges, perim, skipped, outside, runs = {}, [0] * rows, 0, 0, 0
    for y in range(h):
        for x in range(w):
            u = int(plane[y, x])
            if flags & SKIP and u == skip_value:
                skipped += 1
            elif u >= rows:
                outside += 1
            p = val(y, x)
            if p is not None:
                for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                    yy, xx = y + dy, x + dx
                    if not (0 <= yy < h and 0 <= xx < w) or val(yy, xx) != p:
                        perim[p] += 1
            for eid, yy, xx in ((2 * (y * w + x), y, x + 1), (2 * (y * w + x) + 1, y + 1, x)):
                if yy < h and xx < w and border(p, val(yy, xx)):
                    q = val(yy, xx)
                    e = edges.setdefault((min(p, q), max(p, q)), [0, eid])
                    e[0] += 1
                    e[1] = min(e[1], eid)
    # R from its definition: walk every line of edges and count the maximal sequences of equal ordered pairs
    for y in range(h - 1):  # the edges between rows y and y+1, along x
        prev = None
        for x in range(w):
            cur = (val(y, x), val(y + 1, x)) if border(val(y, x), val(y + 1, x)) else None
            if cur is not None and cur != prev:
                runs += 1
            prev = cur
    for x in range(w - 1):  # the edges between columns x and x+1, along y
        prev = None
        for y in range(h):
            cur = (val(y, x), val(y, x + 1)) if border(val(y, x), val(y, x + 1)) else None
            if cur is not None and cur != prev:
                runs += 1
            prev = cur
    pair_list = [(a, b, n, f) for (a, b), (n, f) in edges.items()]
    return _finish(pair_list, np.array(perim, np.uint32), rows, runs, skipped, outside, pair_rows, pair_slots, want_pairs)


def _sieve_out(klass, labels, table, n, n_regions, table_rows, cls, into, rnd, bord, small, rounds, max_rounds, last_resolved, n_pairs, over):
    klass = np.asarray(klass, np.uint8)
    labels = np.asarray(labels)
    rows = np.zeros((n, SIEVE_ROW_WORDS), np.uint32)
    final = np.array([cls[r] if cls[r] is not None else int(table[r, R.CLASS]) for r in range(n)], np.int64)
    rows[:, S_CLASS], rows[:, S_INTO], rows[:, S_BORDER] = final, into, bord
    rows[:, S_ROUND] = [NONE if x is None else x for x in rnd]
    out = klass.copy()
    live = labels < n
    out[live] = final[labels[live]].astype(np.uint8)
    absorbed = sum(1 for r in range(n) if small[r] and cls[r] is not None)
    stranded = sum(small) - absorbed
    changed = sum(int(table[r, R.PIXELS]) for r in range(n) if small[r] and cls[r] is not None and cls[r] != int(table[r, R.CLASS]))
    counts = np.zeros(SIEVE_COUNT_WORDS, np.uint32)
    counts[:7] = n, sum(small), absorbed, stranded, rounds, changed, n_pairs
    counts[S_STATUS] = ((S_OVERFLOW if over else 0) | (S_ROUNDS_EXHAUSTED if last_resolved == max_rounds and stranded else 0) |
                        (S_TABLE_SHORT if n_regions > table_rows else 0))
    return Sieved(out, rows, counts)


def _sieve(adj_fn, klass, labels, table, n_regions, table_rows, min_pixels, max_rounds, pair_slots):
    table_rows = len(table) if table_rows is None else table_rows
    assert 0 <= max_rounds <= MAX_ROUNDS
    max_rounds = max_rounds or DEFAULT_ROUNDS
    n = min(n_regions, table_rows)
    adj = adj_fn(labels, n, pair_slots=pair_slots)
    over = bool(adj.counts[STATUS] & OVERFLOW)
    small = [int(table[r, R.PIXELS]) < min_pixels for r in range(n)]
    cls = [None if small[r] else int(table[r, R.CLASS]) for r in range(n)]
    into, rnd, bord = list(range(n)), [None if s else 0 for s in small], [0] * n
    return adj, over, n, small, cls, into, rnd, bord, max_rounds, table_rows


def sieve(klass, labels, table, n_regions, table_rows=None, min_pixels=0, max_rounds=0, pair_slots=0):
    adj, over, n, small, cls, into, rnd, bord, max_rounds, table_rows = _sieve(adjacency, klass, labels, table, n_regions, table_rows, min_pixels,
                                                                              max_rounds, pair_slots)
    nb = {}
    for a, b, border, _ in adj.pairs.tolist():
        nb.setdefault(a, []).append((border, b))
        nb.setdefault(b, []).append((border, a))
    rounds = last = 0
    for t in range(1, max_rounds + 1):
        if over:
            break
        won = {}
        for r in range(n):
            if cls[r] is None:
                cand = [(border, -q) for border, q in nb.get(r, ()) if cls[q] is not None]
                if cand:
                    won[r] = max(cand)
        if not won:
            break
        for r, (border, mq) in won.items():
            cls[r], into[r], rnd[r], bord[r] = cls[-mq], into[-mq], t, border
        rounds = last = t
    # (the resolutions of a round read only what earlier rounds resolved: `won` is complete before anything is written)
    return _sieve_out(klass, labels, table, n, n_regions, table_rows, cls, into, rnd, bord, small, rounds, max_rounds, last, int(adj.counts[PAIRS]), over)


def brute_sieve(klass, labels, table, n_regions, table_rows=None, min_pixels=0, max_rounds=0, pair_slots=0):
    adj, over, n, small, cls, into, rnd, bord, max_rounds, table_rows = _sieve(brute_adjacency, klass, labels, table, n_regions, table_rows,
                                                                              min_pixels, max_rounds, pair_slots)
    rounds = last = 0
    for t in range(1, max_rounds + 1):
        if over:
            break
        before = list(cls)
        any_won = False
        for r in range(n):
            if before[r] is not None:
                continue
            best = None
            for a, b, border, _ in adj.pairs.tolist():  # every pair, for every region
                for me, q in ((a, b), (b, a)):
                    if me == r and before[q] is not None and (best is None or border > best[0] or (border == best[0] and q < best[1])):
                        best = (border, q)
            if best is not None:
                cls[r], into[r], rnd[r], bord[r] = before[best[1]], into[best[1]], t, best[0]
                any_won = True
        if not any_won:
            break
        rounds = last = t
    return _sieve_out(klass, labels, table, n, n_regions, table_rows, cls, into, rnd, bord, small, rounds, max_rounds, last, int(adj.counts[PAIRS]), over)


def sieve_plane(klass, connectivity=R.CONNECT_8, min_pixels=0, max_rounds=0, pair_slots=0, fn=None):
    """Regions (min_pixels = 0, no skip) then Sieve, as the frame calls do -> (Sieved, labels, table, n)"""
    labels, table, n = R.label(klass, connectivity=connectivity)
    return (fn or sieve)(klass, labels, table, n, min_pixels=min_pixels, max_rounds=max_rounds, pair_slots=pair_slots), labels, table, n
