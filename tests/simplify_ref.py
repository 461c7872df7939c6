"""Reference of Simplify (Douglas-Peucker on Outlines' loops) for the tests: numpy and plain Python only, no product code.

It applies the rule of include/infur_hip.h literally and sequentially.  For one loop v_0 .. v_{n-1}, with v_n := v_0:

* vertex 0 is kept; B, the smallest index in 1 .. n-1 that maximises |v_i - v_0|^2, is kept;
* Split(a, c) runs for (0, B) and (B, n).  With c - a < 2 nothing happens.  Otherwise, for a < i < c,
  D_i = ((x_c - x_a)(y_i - y_a) - (y_c - y_a)(x_i - x_a))^2 and L = |v_c - v_a|^2; when L == 0 (the loop touches itself),
  D_i = |v_i - v_a|^2 and L = 1.  m is the smallest i with maximal D_i; when 256 * D_m > tol16^2 * L, m is kept and Split(a, m)
  and Split(m, c) run;
* the kept vertices come out in their original order.

Python integers do not overflow, so nothing here depends on the 64-bit bound the header states.

``emulate`` is the second implementation: the device kernels' lane logic (simplify.hip) in numpy -- the strided argmax with its
tie order, the register stack, the rank of the flag scan, emit -- which must equal the sequential rule.
"""
import numpy as np

OFFSET, COUNT, VALUE, START, WORDS = 0, 1, 2, 3, 4
STATUS_TRUNCATED, STATUS_MALFORMED = 1, 2
MAX_COORD = 8191


def _xy(ids, w):
    """vertex ids -> python lists x, y; a Y above 8191 (no plane the call accepts has one) reads as 8191"""
    ids = np.asarray(ids, np.int64)
    return (ids % (w + 1)).tolist(), np.minimum(ids // (w + 1), MAX_COORD).tolist()


def keep_loop(x, y, tol16):
    """the indices of the kept vertices of one loop given as lists x, y (n >= 2), ascending.  (Segments of more than 256 vertices are
    evaluated in numpy int64 instead of Python integers, for speed: cross^2 < 2^54 there, and argmax takes the first maximum.)"""
    n = len(x)
    x, y = x + x[:1], y + y[:1]
    nx, ny = (np.array(x, np.int64), np.array(y, np.int64)) if n > 256 else (None, None)
    d0 = [(x[i] - x[0]) ** 2 + (y[i] - y[0]) ** 2 for i in range(1, n)]
    b = 1 + d0.index(max(d0))
    kept = {0, b}
    todo = [(0, b), (b, n)]
    t2 = tol16 * tol16
    while todo:
        a, c = todo.pop()
        if c - a < 2:
            continue
        ex, ey = x[c] - x[a], y[c] - y[a]
        length = ex * ex + ey * ey
        if c - a > 256:
            dx, dy = nx[a + 1:c] - x[a], ny[a + 1:c] - y[a]
            d = (ex * dy - ey * dx) ** 2 if length else dx * dx + dy * dy
            at = int(np.argmax(d))
            dm, m = int(d[at]), a + 1 + at
        else:
            if length == 0:
                d = [(x[i] - x[a]) ** 2 + (y[i] - y[a]) ** 2 for i in range(a + 1, c)]
            else:
                d = [(ex * (y[i] - y[a]) - ey * (x[i] - x[a])) ** 2 for i in range(a + 1, c)]
            dm = max(d)
            m = a + 1 + d.index(dm)
        if 256 * dm > t2 * (length or 1):
            kept.add(m)
            todo += [(a, m), (m, c)]
    return sorted(kept)


def simplify(loops, vertices, counts, w, tol16, loops_rows_in=None, vertex_rows_in=None, keep_fn=keep_loop):
    """Outlines' (loops [*, 4], vertices [*], counts [>= 2]) of a plane of width w -> (loops_out u32 [n_loops, 4], vertices_out u32
    [n_vertices'], counts_out u32 [4] = n_loops, n_vertices', n_degenerate, status).  The rows default to the arrays' lengths.
    Truncated input (status bit 0): no loops, no vertices, counts_out = {counts[0], 0, 0, 1}."""
    assert 0 < w <= MAX_COORD and 0 <= tol16 <= 65535
    loops = np.asarray(loops, np.uint32).reshape(-1, WORDS)
    vertices = np.asarray(vertices, np.uint32).reshape(-1)
    lrows = len(loops) if loops_rows_in is None else loops_rows_in
    vrows = len(vertices) if vertex_rows_in is None else vertex_rows_in
    nl, nv = int(counts[0]), int(counts[1])
    if nl > lrows or nv > vrows:
        return np.zeros((0, WORDS), np.uint32), np.zeros(0, np.uint32), np.array([nl, 0, 0, STATUS_TRUNCATED], np.uint32)
    keep = np.zeros(nv, bool)
    status = 0
    well = []
    for off, cnt, _, _ in loops[:nl].tolist():
        ok = cnt >= 2 and off + cnt <= nv
        well.append(ok)
        if not ok:
            status |= STATUS_MALFORMED
            continue
        x, y = _xy(vertices[off:off + cnt], w)
        keep[off + np.array(keep_fn(x, y, tol16), np.int64)] = True
    # a kept vertex's place is its rank among the kept; a record's OFFSET' the rank at its OFFSET: with Outlines' records, which lie
    # back to back, that is the prefix sum of COUNT'
    rank = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    out = np.zeros((nl, WORDS), np.uint32)
    for i, (off, cnt, val, start) in enumerate(loops[:nl].tolist()):
        out[i] = (rank[min(off, nv)], rank[off + cnt] - rank[off] if well[i] else 0, val, start)
    n_deg = int((out[:, COUNT] < 3).sum())
    return out, vertices[:nv][keep].copy(), np.array([nl, int(rank[nv]), n_deg, status], np.uint32)


def check_invariants(loops, vertices, counts, w, tol16, loops_out, vertices_out, counts_out):
    """the facts that follow from the rule, for well-formed input that is all there"""
    loops, vertices = np.asarray(loops, np.uint32).reshape(-1, WORDS), np.asarray(vertices, np.uint32)
    nl = int(counts[0])
    assert counts_out[0] == nl and counts_out[3] == 0 and loops_out.shape == (nl, WORDS) and vertices_out.shape == (int(counts_out[1]),)
    cnt2 = loops_out[:, COUNT].astype(np.int64)
    assert (loops_out[:, OFFSET] == np.cumsum(cnt2) - cnt2).all() and int(cnt2.sum()) == len(vertices_out)  # OFFSET' is the prefix sum
    assert (loops_out[:, [VALUE, START]] == loops[:nl][:, [VALUE, START]]).all()
    assert int(counts_out[2]) == int((cnt2 < 3).sum())
    t2 = tol16 * tol16
    for (off, cnt, _, _), (off2, c2, _, _) in zip(loops[:nl].tolist(), loops_out.tolist()):
        src, dst = vertices[off:off + cnt].tolist(), vertices_out[off2:off2 + c2].tolist()
        assert 2 <= c2 <= cnt and dst[0] == src[0]
        # a subsequence: the kept indices, found greedily (a saddle vertex may occur twice in a loop; the later checks then say
        # whether the choice was right)
        idx, at = [], 0
        for t in dst:
            at = src.index(t, at)
            idx.append(at)
            at += 1
        x, y = _xy(src, w)
        x, y = x + x[:1], y + y[:1]
        for a, c in zip(idx, idx[1:] + [cnt]):
            ex, ey = x[c] - x[a], y[c] - y[a]
            length = ex * ex + ey * ey
            for i in range(a + 1, c):
                d = (ex * (y[i] - y[a]) - ey * (x[i] - x[a])) ** 2 if length else (x[i] - x[a]) ** 2 + (y[i] - y[a]) ** 2
                assert 256 * d <= t2 * (length or 1), (off, a, i, c)


# ---------------------------------------------------------------- the kernels' lane logic
LANES = 64


def _wave_argmax(key_d, key_i):
    """xor-butterfly over 64 lanes of the key (D, -index): the larger D wins, the smaller index on a tie"""
    d, i = list(key_d), list(key_i)
    step = 32
    while step:
        nd, ni = list(d), list(i)
        for lane in range(LANES):
            od, oi = d[lane ^ step], i[lane ^ step]
            if od > d[lane] or (od == d[lane] and oi < i[lane]):
                nd[lane], ni[lane] = od, oi
        d, i = nd, ni
        step >>= 1
    assert len(set(d)) == 1 and len(set(i)) == 1  # every lane ends with the same answer
    return d[0], i[0]


def _strided_argmax(fn, lo, hi):
    """every lane walks lo + lane, lo + lane + 64, .. < hi and keeps its first maximum of fn; an idle lane holds (0, 2^32 - 1)"""
    key_d, key_i = [0] * LANES, [0xFFFFFFFF] * LANES
    for lane in range(LANES):
        first = True
        for i in range(lo + lane, hi, LANES):
            v = fn(i)
            if first or v > key_d[lane]:
                key_d[lane], key_i[lane], first = v, i, False
    return _wave_argmax(key_d, key_i)


def keep_loop_lanes(x, y, tol16):
    """keep_loop as the keep kernel computes it: strided argmax, the larger half pushed on a stack of one entry per lane"""
    n = len(x)
    x, y = x + x[:1], y + y[:1]
    _, b = _strided_argmax(lambda i: (x[i] - x[0]) ** 2 + (y[i] - y[0]) ** 2, 1, n)
    kept = {0, b}
    stack = [None] * LANES
    stack[0], sp = (b, n), 1
    a, c = 0, b
    t2 = tol16 * tol16
    while True:
        if c - a < 2:
            if sp == 0:
                break
            sp -= 1
            a, c = stack[sp]
            continue
        ex, ey = x[c] - x[a], y[c] - y[a]
        length = ex * ex + ey * ey
        if length == 0:
            dm, m = _strided_argmax(lambda i: (x[i] - x[a]) ** 2 + (y[i] - y[a]) ** 2, a + 1, c)
            length = 1
        else:
            dm, m = _strided_argmax(lambda i: (ex * (y[i] - y[a]) - ey * (x[i] - x[a])) ** 2, a + 1, c)
        assert 256 * dm < 1 << 63 and t2 * length < 1 << 63  # the header's bound
        if 256 * dm > t2 * length:
            kept.add(m)
            assert sp < LANES
            if m - a >= c - m:  # the larger half waits, the smaller is next: the stack stays below log2(n) + 2 entries
                stack[sp], a = (a, m), m
            else:
                stack[sp], c = (m, c), m
            sp += 1
            assert sp <= max(2, n).bit_length() + 1
        else:
            c = a  # done with this segment
    return sorted(kept)


_LANES_SEEN = {}


def emulate(loops, vertices, counts, w, tol16, loops_rows_in=None, vertex_rows_in=None, loops_rows_out=None, vertex_rows_out=None,
            block=1024):
    """the launches of simplify.hip in numpy on buffers of the declared rows -> (loops_out [loops_rows_out, 4], vertices_out
    [vertex_rows_out], counts_out [4]); what a launch leaves alone holds 0xA5A5A5A5"""
    loops = np.asarray(loops, np.uint32).reshape(-1, WORDS)
    vertices = np.asarray(vertices, np.uint32).reshape(-1)
    lrows = len(loops) if loops_rows_in is None else loops_rows_in
    vrows = len(vertices) if vertex_rows_in is None else vertex_rows_in
    loops, vertices = loops[:lrows], vertices[:vrows]  # no lane reads beyond the declared rows
    c0, c1 = int(counts[0]), int(counts[1])
    truncated = c0 > lrows or c1 > vrows
    nl, nv = (0, 0) if truncated else (c0, c1)
    # keep: one wave per loop
    keep = np.zeros(vrows, np.uint8)  # (the memset)
    for i in range(nl):
        off, cnt = int(loops[i, OFFSET]), int(loops[i, COUNT])
        if cnt < 2 or off + cnt > nv:
            continue
        x, y = _xy(vertices[off:off + cnt], w)
        # (the rule sees coordinate differences only: a loop of a shape seen before -- a noise plane has thousands of unit squares --
        # is not walked lane by lane again)
        key = (tuple(t - x[0] for t in x), tuple(t - y[0] for t in y), tol16)
        if key not in _LANES_SEEN:
            _LANES_SEEN[key] = np.array(keep_loop_lanes(x, y, tol16), np.int64)
        keep[off + _LANES_SEEN[key]] = 1
    # sums, partials, rank over the positions 0 .. vrows (one more than the vertices: rank[nv] is the total)
    flag = np.zeros(vrows + 1, np.int64)
    flag[:nv] = keep[:nv]
    nb = (vrows + 1 + block - 1) // block
    sums = np.add.reduceat(np.concatenate([flag, np.zeros(nb * block - len(flag), np.int64)]), np.arange(nb) * block)
    base = np.cumsum(sums) - sums
    rank = np.zeros(vrows + 1, np.int64)
    for blk in range(nb):
        f = flag[blk * block:(blk + 1) * block]
        rank[blk * block:blk * block + len(f)] = base[blk] + np.cumsum(f) - f
    n_out = int(sums.sum())
    lro = nl if loops_rows_out is None else loops_rows_out
    vro = n_out if vertex_rows_out is None else vertex_rows_out
    vout = np.full(vro, 0xA5A5A5A5, np.uint32)
    for p in np.flatnonzero(flag).tolist():
        if rank[p] < vro:
            vout[rank[p]] = vertices[p]
    # records: one lane per loop
    lout = np.full((lro, WORDS), 0xA5A5A5A5, np.uint32)
    n_deg = n_bad = 0
    for i in range(nl):
        off, cnt, val, start = (int(t) for t in loops[i])
        bad = cnt < 2 or off + cnt > nv
        c2 = 0 if bad else int(rank[off + cnt] - rank[off])
        n_deg += c2 < 3
        n_bad += bad
        if i < lro:
            lout[i] = (rank[min(off, nv)], c2, val, start)
    return lout, vout, np.array([c0, n_out, n_deg, (1 if truncated else 0) | (2 if n_bad else 0)], np.uint32)


def stairs(k):
    """a right triangle of class 1 on class 0 whose hypotenuse is a staircase of k unit steps: k x k pixels, row y holds pixels
    0 .. y.  Skipping class 0 leaves one loop of 2k + 2 vertices whose 45-degree corners tie exactly in D"""
    p = np.zeros((k, k), np.uint8)
    for y in range(k):
        p[y, :y + 1] = 1
    return p


def comb(h, w, seed=5):
    """one region of class 1: a spine along row 0, a tooth down every third column, a barb on every other row of each tooth.  The
    teeth have pseudo-random lengths between h / 2 and h - 1, so that the farthest tip of a segment splits it at a random place
    and the recursion stays about 2 * log2(teeth) deep.  (Teeth of one length tie in D: the rule then peels them one by one, the
    quadratic worst case.)  Skipping class 0 leaves one loop of about h * w / 2 vertices"""
    p = np.zeros((h, w), np.uint8)
    p[0] = 1
    length = np.random.RandomState(seed).randint(h // 2, h, size=(w + 2) // 3)
    rows = np.arange(h)[:, None]
    tooth = rows <= length[None, :]
    p[:, 0::3] |= tooth[:, :len(p[0, 0::3])]
    barb = tooth & (rows % 2 == 0) & (rows >= 2)
    n1 = len(p[0, 1::3])
    p[:, 1::3] |= barb[:, :n1]
    return p
