"""Adjacency and Sieve on the GPU: the pair records, row tables and counts of ``infur_adjacency*``, the cleaned plane, rows and
counts of ``infur_sieve*`` and of the fused ``infur_frame_sieve*`` against tests/sieve_ref.py.  Everything is an integer, exact and
a function of the inputs alone, so every comparison is ``==`` on whole arrays.  Every output buffer is filled with a poison byte
first: what a call must leave alone still holds it afterwards, and what it must write owes nothing to an initialisation."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import coverage_ref as V  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import sieve_ref as S  # noqa: E402
from test_gpu_compare import FRAME_H, FRAME_W, POISON, Dev  # noqa: E402
from test_gpu_coverage import dev_coverage  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd import weights as W  # noqa: E402
from infur_amd.processors import (Adjacency, AdjacencyOut, Context, FramePath, Model, ModelCmd, Regions, RegionsOut, Sieve,  # noqa: E402
                                  SieveOut, adjacency_graph, sieve_summary)

pytestmark = pytest.mark.gpu

RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
NONE = 0xFFFFFFFF
ADJ_OUTPUTS = ("pairs", "rows", "counts")
SIEVE_OUTPUTS = ("klass_out", "rows", "counts")
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (2, 130), (13, 70), (33, 63), (40, 130), (65, 129))


# --------------------------------------------------------------------------- #
# helpers
# --------------------------------------------------------------------------- #
def dev_adjacency(ctx, plane, rows, flags=0, skip_value=0, pair_rows=0, pair_slots=0, want=ADJ_OUTPUTS):
    """infur_adjacency_dev on poisoned device buffers -> {pairs [pair_rows, 4] as the buffer holds it, rows [rows, 4], counts [8]},
    None for what was not wanted (and that buffer is checked to be untouched)"""
    h, w = plane.shape
    d = Dev(ctx, plane=plane.nbytes, pairs=pair_rows * 16, rows=rows * 16, counts=32)
    try:
        d.put("plane", plane)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_adjacency_dev(ctx.h, d.ptr["plane"], plane.dtype.itemsize, h, w, flags, skip_value, rows, p("pairs"), pair_rows, p("rows"),
                                            p("counts"), pair_slots))
        ctx.synchronize()
        assert d.get("plane").tobytes() == plane.tobytes()  # the input is an input
        got = {"pairs": d.get("pairs").view(np.uint32).reshape(pair_rows, 4), "rows": d.get("rows").view(np.uint32).reshape(rows, 4),
               "counts": d.get("counts").view(np.uint32)}
        for name in ADJ_OUTPUTS:
            if name not in want:
                assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
                got[name] = None
        return got
    finally:
        d.free()


_PLANES = {}


def _key(p):
    key = (p.shape, p.dtype.str, p.tobytes())
    _PLANES.setdefault(key, p)
    return key


@functools.lru_cache(maxsize=None)
def _adj_reference(key, rows, flags, skip_value, pair_rows, pair_slots, want_pairs):
    return S.adjacency(_PLANES[key], rows, flags, skip_value, pair_rows, pair_slots, want_pairs)


def adj_reference(plane, rows, flags=0, skip_value=0, pair_rows=0, pair_slots=0, want_pairs=True):
    """the reference's answer, computed once per plane and setting, and left unchanged"""
    return _adj_reference(_key(plane), rows, flags, skip_value, pair_rows, pair_slots, want_pairs)


def check_adjacency(ctx, plane, rows, name="", want=ADJ_OUTPUTS, **kw):
    ref = adj_reference(plane, rows, want_pairs="pairs" in want, **kw)
    got = dev_adjacency(ctx, plane, rows, want=want, **kw)
    print(f"{name} {plane.shape[0]}x{plane.shape[1]} {plane.dtype} rows {rows} {kw}: counts {ref.counts.tolist()}")
    tag = (name, plane.shape, str(plane.dtype), rows, kw)
    if got["counts"] is not None:
        assert (got["counts"] == ref.counts).all(), tag + (got["counts"].tolist(), ref.counts.tolist())
    if got["rows"] is not None:
        assert (got["rows"] == ref.rows).all(), tag
    if got["pairs"] is not None:
        n = len(ref.pairs)
        assert (got["pairs"][:n] == ref.pairs).all(), tag
        assert (got["pairs"][n:].view(np.uint8) == POISON).all(), tag  # what lies behind the records is left alone
    return ref


@functools.lru_cache(maxsize=None)
def _label(key, conn, min_pixels):
    return R.label(_PLANES[key], connectivity=conn, min_pixels=min_pixels)


def label_of(k, conn, min_pixels=0):
    return _label(_key(k), conn, min_pixels)


@functools.lru_cache(maxsize=None)
def _sieve_reference(key, conn, label_min, table_rows, min_pixels, max_rounds, pair_slots):
    labels, table, n = _label(key, conn, label_min)
    return S.sieve(_PLANES[key], labels, table, n, table_rows, min_pixels, max_rounds, pair_slots)


def sieve_reference(k, conn, min_pixels, max_rounds=0, pair_slots=0, table_rows=None, label_min=0):
    return _sieve_reference(_key(k), conn, label_min, table_rows, min_pixels, max_rounds, pair_slots)


def dev_sieve(ctx, k, conn, min_pixels, max_rounds=0, pair_slots=0, table_rows=None, label_min=0, want=SIEVE_OUTPUTS, then=None):
    """infur_regions_dev (min_pixels = label_min, no skip), then infur_sieve_dev of what it left on the device, on poisoned buffers
    -> {klass_out [h, w], rows [table_rows, 4] as the buffer holds it, counts [8]}, None for what was not wanted.  then(d): more
    calls on the buffers before they are freed."""
    h, w = k.shape
    rows = h * w if table_rows is None else table_rows
    d = Dev(ctx, klass=h * w, labels=h * w * 4, table=rows * 80, n=4, klass_out=h * w, rows=rows * 16, counts=32)
    try:
        d.put("klass", k)
        P = d.ptr
        ctx.check(ctx.L.infur_regions_dev(ctx.h, P["klass"], None, h, w, conn, label_min, 0, P["labels"], P["table"] if rows else None, rows, P["n"]))
        ctx.synchronize()
        before = {name: d.get(name).tobytes() for name in ("klass", "labels", "table", "n")}
        p = lambda name: P[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_sieve_dev(ctx.h, P["klass"], P["labels"], P["table"], rows, P["n"], h, w, min_pixels, max_rounds, pair_slots,
                                        p("klass_out"), p("rows"), p("counts")))
        ctx.synchronize()
        assert all(d.get(name).tobytes() == v for name, v in before.items())  # the inputs are inputs
        got = {"klass_out": d.get("klass_out").reshape(h, w), "rows": d.get("rows").view(np.uint32).reshape(rows, 4),
               "counts": d.get("counts").view(np.uint32)}
        for name in SIEVE_OUTPUTS:
            if name not in want:
                assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
                got[name] = None
        if then:
            got["then"] = then(d)
        return got
    finally:
        d.free()


def check_sieve(ctx, k, conn, min_pixels, name="", want=SIEVE_OUTPUTS, **kw):
    ref = sieve_reference(k, conn, min_pixels, **kw)
    got = dev_sieve(ctx, k, conn, min_pixels, want=want, **kw)
    print(f"{name} {k.shape[0]}x{k.shape[1]} conn {conn} min_pixels {min_pixels} {kw}: counts {ref.counts.tolist()}")
    tag = (name, k.shape, conn, min_pixels, kw)
    if got["counts"] is not None:
        assert (got["counts"] == ref.counts).all(), tag + (got["counts"].tolist(), ref.counts.tolist())
    if got["klass_out"] is not None:
        assert (got["klass_out"] == ref.klass_out).all(), tag
    if got["rows"] is not None:
        n = len(ref.rows)
        assert (got["rows"][:n] == ref.rows).all(), tag
        assert (got["rows"][n:].view(np.uint8) == POISON).all(), tag  # rows at or beyond n are left alone
    return ref, got


def planes_of(h, w):
    yield "smooth", R.smooth(h, w, seed=h + w, classes=5, cell=4)
    yield "noise", R.noise(h, w, 4, seed=w)
    yield "stripes", R.stripes(h, w)
    yield "checkerboard", R.checkerboard(h, w)


# --------------------------------------------------------------------------- #
# 1. infur_adjacency_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", SHAPES)
def test_adjacency_equals_the_reference(ctx, shape):
    assert ctx.L.infur_features() & _lib.FEATURE_SIEVE  # (the first line: fails on a library without the feature)
    h, w = shape
    for name, k in planes_of(h, w):
        top = int(k.max())
        most = 2 * h * w  # no plane has more pairs than edges
        check_adjacency(ctx, k, top + 1, name, pair_rows=most)
        check_adjacency(ctx, k.astype(np.uint32), top + 1, name, pair_rows=most)
        check_adjacency(ctx, k, max(top, 1), name, pair_rows=most)  # rows cut the largest value off
        check_adjacency(ctx, k, top + 2, name, flags=S.SKIP, skip_value=0, pair_rows=most)
        labels, _, n = label_of(k, R.CONNECT_8 if (h + w) & 1 else R.CONNECT_4)
        check_adjacency(ctx, labels, n, name + " labels", pair_rows=most)
        check_adjacency(ctx, labels, max(n - 1, 0), name + " labels", pair_rows=most)
    filtered, _, n = label_of(R.noise(h, w, 4, seed=w), R.CONNECT_4, 3)
    check_adjacency(ctx, filtered, n + 1, "filtered labels", flags=S.SKIP, skip_value=NONE, pair_rows=2 * h * w)


def test_adjacency_output_sizes_and_subsets(ctx):
    k = R.smooth(40, 130, seed=2, classes=6, cell=8)
    labels, _, n = label_of(k, R.CONNECT_8)
    full = adj_reference(labels, n, pair_rows=4096)
    pairs = int(full.counts[S.PAIRS])
    assert pairs > 8 and full.counts[S.STATUS] == 0
    for pair_rows in (0, 3, pairs - 1, pairs, pairs + 7):  # none, short and ample
        ref = check_adjacency(ctx, labels, n, "sizes", pair_rows=pair_rows)
        assert ref.counts[S.WRITTEN] == min(pairs, pair_rows) and bool(ref.counts[S.STATUS] & S.TRUNCATED) == (pair_rows < pairs)
    for want in (("pairs",), ("rows",), ("counts",), ("pairs", "counts"), ("rows", "counts"), ("pairs", "rows")):
        check_adjacency(ctx, labels, n, "subset", want=want, pair_rows=pairs + 2)
    ref = check_adjacency(ctx, labels, n, "no pairs", want=("rows", "counts"), pair_rows=5)  # records not wanted: nothing is truncated
    assert ref.counts[S.WRITTEN] == 0 == ref.counts[S.STATUS]
    check_adjacency(ctx, labels, 0, "no rows", pair_rows=4)


def test_adjacency_overflow_and_the_exact_edge_of_the_rule(ctx):
    k = R.noise(33, 63, 3, seed=1)
    ref = check_adjacency(ctx, k, 3, "overflow", pair_rows=16, pair_slots=64)
    assert ref.counts[S.STATUS] == S.OVERFLOW and 2 * int(ref.counts[S.RUNS]) > 64 and (ref.rows[:, :3] == [0, NONE, 0]).all()
    assert (ref.rows[:, S.PERIMETER] == adj_reference(k, 3, pair_rows=16).rows[:, S.PERIMETER]).all()
    labels, _, n = label_of(k, R.CONNECT_4)
    check_adjacency(ctx, labels, n, "overflow labels", pair_rows=16, pair_slots=1024)
    alt = (np.arange(33) % 2).astype(np.uint8)[None]  # 2 R == 64 exactly: no overflow
    ref = check_adjacency(ctx, alt, 2, "exact", pair_rows=4, pair_slots=64)
    assert ref.counts[S.RUNS] == 32 and ref.counts[S.STATUS] == 0 and ref.pairs.tolist() == [[0, 1, 32, 0]]
    alt = (np.arange(34) % 2).astype(np.uint8)[None]
    assert check_adjacency(ctx, alt, 2, "one more", pair_rows=4, pair_slots=64).counts[S.STATUS] == S.OVERFLOW
    labels, _, n = label_of(R.stripes(5, 64), R.CONNECT_4)
    ref = check_adjacency(ctx, labels, n, "stripes", pair_rows=64, pair_slots=128)
    assert ref.counts[S.RUNS] == 63 == ref.counts[S.PAIRS] and (ref.pairs[:, S.BORDER] == 5).all()


def test_adjacency_calls_are_repeatable(ctx):
    k = R.noise(65, 129, 5, seed=4)
    labels, _, n = label_of(k, R.CONNECT_4)
    first = dev_adjacency(ctx, labels, n, pair_rows=16384)
    dev_adjacency(ctx, R.smooth(40, 130, seed=1, classes=4, cell=8), 4, pair_rows=64)  # another call in between
    second = dev_adjacency(ctx, labels, n, pair_rows=16384)
    assert all(first[name].tobytes() == second[name].tobytes() for name in ADJ_OUTPUTS)


def test_adjacency_rules_host_call_and_processor(ctx):
    L, h = ctx.L, ctx.h
    k = R.smooth(13, 70, seed=5, classes=5, cell=4)
    pairs, rows, counts = np.full((64, 4), 9, np.uint32), np.full((5, 4), 9, np.uint32), np.full(8, 9, np.uint32)
    p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731

    def call(elem=1, hh=13, ww=70, flags=0, skip=0, nrows=5, plane=k, pr=pairs, pair_rows=64, ro=rows, cn=counts, slots=0):
        return L.infur_adjacency(h, p(plane), elem, hh, ww, flags, skip, nrows, p(pr), pair_rows, p(ro), p(cn), slots)

    for bad, word in ((dict(elem=2), "elem_bytes"), (dict(flags=2), "unknown adjacency flags"), (dict(flags=1, skip=256), "skip_value"),
                      (dict(hh=65536), "65535"), (dict(slots=48), "pair_slots"), (dict(slots=32), "pair_slots"),
                      (dict(pr=None, ro=None, cn=None), "no output wanted"), (dict(pr=None, nrows=0, cn=None), "no output wanted"),
                      (dict(plane=None), "no plane pointer")):
        assert call(**bad) == _lib.E_INVALID_ARG and word in ctx.last_error(), bad
    assert all((x == 9).all() for x in (pairs, rows, counts))  # a rejected call touches no output
    assert call(elem=2, slots=3) == _lib.E_INVALID_ARG and "elem_bytes" in ctx.last_error()  # the order of the checks
    assert call() == _lib.OK
    ref = adj_reference(k, 5, pair_rows=64)
    n = len(ref.pairs)
    assert (pairs[:n] == ref.pairs).all() and (pairs[n:] == 9).all() and (rows == ref.rows).all() and (counts == ref.counts).all()
    assert call(hh=0, plane=None) == _lib.OK and counts.tolist() == [0] * 8 and (rows == [0, NONE, 0, 0]).all()
    out = AdjacencyOut(rows=5, pair_rows=64)
    Adjacency(ctx).advance(k, out)
    assert (out.pairs == ref.pairs).all() and (out.table == ref.rows).all() and (out.counts == ref.counts).all()
    g = adjacency_graph(out.pairs, 5)
    assert all(len(g[v]) == ref.rows[v, S.DEGREE] and (not g[v] or g[v][0] == (ref.rows[v, S.LONGEST], ref.rows[v, S.ROW_BORDER])) for v in range(5))
    out = AdjacencyOut(rows=6, pair_rows=64)
    Adjacency(ctx, skip_value=0).advance(k.astype(np.uint32), out)
    ref = adj_reference(k.astype(np.uint32), 6, flags=S.SKIP, skip_value=0, pair_rows=64)
    assert (out.pairs == ref.pairs).all() and (out.table == ref.rows).all() and (out.counts == ref.counts).all()


# --------------------------------------------------------------------------- #
# 2. infur_regions_dev -> infur_sieve_dev against the reference
# --------------------------------------------------------------------------- #
FACTS = {"smooth": (lambda: R.smooth(40, 70, seed=3, classes=6, cell=8), 64), "noise5": (lambda: R.noise(65, 129, 5, seed=4), 8),
         "noise3": (lambda: R.noise(33, 63, 3, seed=1), 64), "single": (lambda: R.single(9, 11), 64), "worked": (lambda: S.WORKED, 4)}


@pytest.mark.parametrize("conn", [R.CONNECT_4, R.CONNECT_8])
@pytest.mark.parametrize("fact", sorted(FACTS))
def test_sieve_equals_the_reference(ctx, fact, conn):
    assert ctx.L.infur_features() & _lib.FEATURE_SIEVE
    k, min_pixels = FACTS[fact][0](), FACTS[fact][1]
    ref, _ = check_sieve(ctx, k, conn, min_pixels, fact, max_rounds=64)
    if fact == "smooth" and conn == R.CONNECT_8:
        assert ref.counts.tolist() == [48, 33, 33, 0, 2, 664, 103, 0]
    if fact == "noise3" and conn == R.CONNECT_4:
        assert ref.counts[:6].tolist() == [767, 767, 0, 767, 0, 0] and (ref.klass_out == k).all()
    if fact == "worked":
        assert ref.counts.tolist() == [5, 3, 3, 0, 2, 5, 4, 0]
    for mp in (0, 1, 2):
        check_sieve(ctx, k, conn, mp, fact)


@pytest.mark.parametrize("shape", SHAPES[:7])
def test_sieve_on_the_edge_shapes(ctx, shape):
    h, w = shape
    for name, k in planes_of(h, w):
        for conn, mp in ((R.CONNECT_4, 2), (R.CONNECT_8, 8)):
            check_sieve(ctx, k, conn, mp, name)


def test_sieve_every_subset_of_the_outputs(ctx):
    k = R.smooth(40, 70, seed=3, classes=6, cell=8)
    for want in (("klass_out",), ("rows",), ("counts",), ("klass_out", "rows"), ("klass_out", "counts"), ("rows", "counts"), SIEVE_OUTPUTS):
        check_sieve(ctx, k, R.CONNECT_8, 64, "subset", want=want)


def test_sieve_single_cases(ctx):
    smooth, noise = R.smooth(40, 70, seed=3, classes=6, cell=8), R.noise(65, 129, 5, seed=4)
    # a short table: the regions beyond it are fixed, and the status says so
    ref, _ = check_sieve(ctx, smooth, R.CONNECT_8, 64, "short", table_rows=20)
    assert ref.counts[S.S_REGIONS] == 20 and ref.counts[S.S_STATUS] & S.S_TABLE_SHORT
    # the NONE pixels of a min_pixels-filtered label plane stay fixed
    ref, got = check_sieve(ctx, smooth, R.CONNECT_8, 64, "filtered", label_min=12)
    none = label_of(smooth, R.CONNECT_8, 12)[0] == NONE
    assert none.any() and (got["klass_out"][none] == smooth[none]).all() and ref.counts[S.S_SMALL] > 0
    # one round
    ref, _ = check_sieve(ctx, S.WORKED, R.CONNECT_4, 4, "one round", max_rounds=1)
    assert ref.counts.tolist() == [5, 3, 2, 1, 1, 4, 4, S.S_ROUNDS_EXHAUSTED]
    # the 17-round case: with room, with exactly 17, with the default 8
    ref, _ = check_sieve(ctx, noise, R.CONNECT_4, 8, "17 rounds", max_rounds=64)
    assert ref.counts[:5].tolist() == [5193, 5162, 5162, 0, 17] and ref.counts[S.S_STATUS] == 0
    ref, _ = check_sieve(ctx, noise, R.CONNECT_4, 8, "17 rounds", max_rounds=17)
    assert ref.counts[S.S_STRANDED] == 0 and ref.counts[S.S_STATUS] == 0
    ref, _ = check_sieve(ctx, noise, R.CONNECT_4, 8, "default rounds")
    assert ref.counts[S.S_ROUNDS] == 8 and ref.counts[S.S_STATUS] == S.S_ROUNDS_EXHAUSTED and ref.counts[S.S_STRANDED] > 0
    # overflow: the plane is copied
    ref, got = check_sieve(ctx, smooth, R.CONNECT_8, 64, "overflow", pair_slots=64)
    assert ref.counts.tolist() == [48, 33, 0, 33, 0, 0, 0, S.S_OVERFLOW] and (got["klass_out"] == smooth).all()
    # two calls give identical bytes
    a, b = dev_sieve(ctx, noise, R.CONNECT_4, 8, max_rounds=64), dev_sieve(ctx, noise, R.CONNECT_4, 8, max_rounds=64)
    assert all(a[name].tobytes() == b[name].tobytes() for name in SIEVE_OUTPUTS)


@pytest.mark.parametrize("conn", [R.CONNECT_4, R.CONNECT_8])
def test_the_invariant_checked_by_regions_on_the_device(ctx, conn):
    """no region of the cleaned plane is smaller than min_pixels, counted by infur_regions_dev on klass_out where Sieve left it"""
    for name, k, mp in (("smooth", R.smooth(40, 70, seed=3, classes=6, cell=8), 64), ("noise5", R.noise(65, 129, 5, seed=4), 8),
                        ("worked", S.WORKED, 4)):
        h, w = k.shape

        def relabel(d, h=h, w=w):
            d.poison("labels", "table", "n")
            ctx.check(ctx.L.infur_regions_dev(ctx.h, d.ptr["klass_out"], None, h, w, conn, 0, 0, d.ptr["labels"], d.ptr["table"], h * w, d.ptr["n"]))
            ctx.synchronize()
            n = int(d.get("n").view(np.uint32)[0])
            return d.get("labels").view(np.uint32).reshape(h, w), d.get("table").view(np.uint64).reshape(h * w, 10)[:n], n

        got = dev_sieve(ctx, k, conn, mp, max_rounds=64, then=relabel)
        assert got["counts"][S.S_STRANDED] == 0, name  # first: no case hides behind it
        labels2, table2, n2 = got["then"]
        ref = sieve_reference(k, conn, mp, max_rounds=64)
        want = R.label(ref.klass_out, connectivity=conn)
        assert n2 == want[2] and (labels2 == want[0]).all() and (table2[:, [R.PIXELS, R.CLASS, R.FIRST]] == want[1][:, [R.PIXELS, R.CLASS, R.FIRST]]).all()
        assert int(table2[:, R.PIXELS].min()) >= mp, (name, conn)
        kept = label_of(k, conn)[1][:, R.PIXELS] >= mp
        mask = kept[label_of(k, conn)[0]]
        assert (got["klass_out"][mask] == k[mask]).all()  # the pixels of kept regions are unchanged


def test_sieve_rules_host_call_and_processor(ctx):
    L, h = ctx.L, ctx.h
    k = R.smooth(40, 70, seed=3, classes=6, cell=8)
    labels, table, n = label_of(k, R.CONNECT_8)
    labels, table = np.ascontiguousarray(labels), np.ascontiguousarray(table)
    out, rows, counts = np.full((40, 70), 9, np.uint8), np.full((n, 4), 9, np.uint32), np.full(8, 9, np.uint32)
    p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731

    def call(hh=40, ww=70, rounds=0, slots=0, kl=k, lb=labels, tb=table, ko=out, ro=rows, cn=counts, mp=64):
        return L.infur_sieve(h, p(kl), p(lb), p(tb), n, n, hh, ww, mp, rounds, slots, p(ko), p(ro), p(cn))

    for bad, word in ((dict(ww=65536), "65535"), (dict(rounds=65), "max_rounds"), (dict(slots=100), "pair_slots"),
                      (dict(ko=None, ro=None, cn=None), "no output wanted"), (dict(kl=None), "no class plane"), (dict(lb=None), "no class plane")):
        assert call(**bad) == _lib.E_INVALID_ARG and word in ctx.last_error(), bad
    assert call(rounds=65, slots=3) == _lib.E_INVALID_ARG and "max_rounds" in ctx.last_error()  # the order of the checks
    assert all((x == 9).all() for x in (out, rows, counts))
    assert call() == _lib.OK
    ref = sieve_reference(k, R.CONNECT_8, 64)
    assert (out == ref.klass_out).all() and (rows == ref.rows).all() and (counts == ref.counts).all()
    assert call(hh=0) == _lib.OK and counts.tolist() == [0] * 8
    # the processors: Regions -> Sieve
    ro = RegionsOut(table_rows=256)
    Regions(ctx, connectivity=8).advance((k, None), ro)
    so = SieveOut()
    Sieve(ctx, min_pixels=64).advance((k, ro.labels, ro.table, ro.n), so)
    assert (so.klass == ref.klass_out).all() and (so.rows == ref.rows).all() and (so.counts == ref.counts).all()
    assert sieve_summary(so.counts)["absorbed"] == 33 and not sieve_summary(so.counts)["overflow"]


# --------------------------------------------------------------------------- #
# 3. the frame calls
# --------------------------------------------------------------------------- #
def frame_reference(klass, conn, min_pixels, flags, max_rounds=0):
    ref = sieve_reference(klass, conn, min_pixels, max_rounds=max_rounds)
    return ref, R.label(ref.klass_out, None, conn, 0, flags)


@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_segments_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    frame = W.synth_frame(FRAME_H, FRAME_W, index=5)
    for factor, conn, flags in ((1.0, 8, 0), (0.5, 4, _lib.REGIONS_SKIP_BACKGROUND)):
        s = fp.advance_segments(frame, factor, decode)
        sizes = np.sort(label_of(s.klass, conn)[1][:, R.PIXELS])
        assert len(sizes) > 1
        mp = int(sizes[len(sizes) // 2 - 1]) + 1  # the threshold from the plane itself: the smaller half of its regions is small
        ref, (labels, table, n) = frame_reference(s.klass, conn, mp, flags, max_rounds=64)
        assert ref.counts[S.S_SMALL] > 0 and ref.counts[S.S_ABSORBED] > 0
        f = fp.advance_sieve(frame, mp, factor, decode, conn, flags, table_rows=4096, max_rounds=64, want_klass=True, want_scaled=True)
        assert (f.klass == s.klass).all() and (f.conf == s.conf).all() and f.scaled.shape == s.klass.shape + (3,)
        assert (f.cleaned == ref.klass_out).all() and (f.counts == ref.counts).all()
        assert f.n == n and (f.labels == labels).all()
        conf_table = R.label(ref.klass_out, s.conf, conn, 0, flags)[1]
        assert (f.table == conf_table).all()
        q = fp.advance_sieve(frame, mp, factor, decode, conn, flags, table_rows=0, max_rounds=64, want_labels=False, want_conf=False)  # no second pass
        assert q.labels is None and q.table is None and (q.cleaned == ref.klass_out).all() and (q.counts == ref.counts).all()
        r = fp.advance_sieve(frame, mp, factor, decode, conn, flags, table_rows=4096, max_rounds=64, want_cleaned=False)  # the cleaned plane in scratch
        assert r.cleaned is None and (r.labels == labels).all() and r.n == n and (r.counts == ref.counts).all()
    lo, _ = model.lowres()  # infur_model_read_lowres still works afterwards
    assert lo.size > 0 and np.isfinite(lo).all()


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    hh, ww, rows = FRAME_H, FRAME_W, 300
    frame = W.synth_frame(hh, ww, index=2)
    s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
    ref, (labels, _, n) = frame_reference(s.klass, 8, 30, 0)
    table = R.label(ref.klass_out, s.conf, 8, 0, 0)[1]
    assert n <= rows
    names = ("klass", "conf", "klass_out", "labels", "table", "n", "counts")
    d = Dev(ctx, bgr=frame.nbytes, klass=hh * ww, conf=hh * ww, klass_out=hh * ww, labels=hh * ww * 4, table=rows * 80, n=4, counts=32)
    try:
        d.put("bgr", frame)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        P = d.ptr
        for want in (names, ("counts",), ("klass_out",), ("labels", "n"), ("table", "conf"), ("klass", "klass_out", "counts"), ("n",)):
            d.poison(*names)
            p = lambda name: P[name] if name in want else None  # noqa: E731
            ctx.check(L.infur_frame_sieve_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 8, 30, 0, p("klass"), p("conf"), hh * ww, p("labels"), hh * ww * 4,
                                              p("table"), rows, p("n"), None, C.byref(ow), C.byref(oh), 0, 0, p("klass_out"), p("counts")))
            ctx.synchronize()
            assert (ow.value, oh.value) == (ww, hh)
            expect = {"klass": s.klass, "conf": s.conf, "klass_out": ref.klass_out, "labels": labels, "n": np.array([n], np.uint32), "counts": ref.counts}
            for name in names:
                got = d.get(name)
                if name not in want:
                    assert (got == POISON).all(), (want, name)
                elif name == "table":
                    assert got[:n * 80].tobytes() == table.tobytes() and (got[n * 80:] == POISON).all(), want
                else:
                    assert got.tobytes() == np.ascontiguousarray(expect[name]).tobytes(), (want, name)
    finally:
        d.free()


def test_fused_rules_and_error_codes(ctx, model):
    """the capacity errors and the check order are infur_frame_regions' own"""
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    npix = 48 * 64
    s = FramePath(ctx).advance_segments(frame, 1.0, RAW)
    klass, out, labels = np.full((48, 64), 9, np.uint8), np.full((48, 64), 9, np.uint8), np.full((48, 64), 9, np.uint32)
    counts, n = np.full(8, 9, np.uint32), np.full(1, 9, np.uint32)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731

    def call(lib=L, handle=h, decode=0, mode=0, factor=1.0, conn=8, flags=0, kl=None, plane_cap=npix, lb=labels, lcap=npix * 4, nr=n, rounds=0, slots=0,
             ko=out, cn=counts, scaled=None):
        return lib.infur_frame_sieve(handle, p(frame), 64, 48, factor, mode, decode, conn, 16, flags, p(kl), None, plane_cap, p(lb), lcap, None, 0, p(nr),
                                     p(scaled), C.byref(ow), C.byref(oh), rounds, slots, p(ko), p(cn))

    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48)
    ref, (want_labels, _, want_n) = frame_reference(s.klass, 8, 16, 0)
    assert (out == ref.klass_out).all() and (counts == ref.counts).all() and (labels == want_labels).all() and n[0] == want_n
    assert call(conn=5) == _lib.E_INVALID_ARG and "connectivity" in ctx.last_error()
    assert call(flags=2) == _lib.E_INVALID_ARG and "regions flags" in ctx.last_error()
    assert call(conn=5, rounds=65) == _lib.E_INVALID_ARG and "connectivity" in ctx.last_error()  # Regions' checks come first
    assert call(rounds=65) == _lib.E_INVALID_ARG and "max_rounds" in ctx.last_error()
    assert call(slots=3) == _lib.E_INVALID_ARG and "pair_slots" in ctx.last_error()
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) != _lib.OK and call(factor=-1.0) == _lib.E_INVALID_SCALE
    assert call(lcap=npix * 4 - 1) == _lib.E_CAPACITY and "label plane" in ctx.last_error()
    assert call(plane_cap=npix - 1) == _lib.E_CAPACITY and "a plane needs" in ctx.last_error()
    assert call(kl=klass, ko=None, plane_cap=npix - 1) == _lib.E_CAPACITY and (klass == 9).all()
    assert call(lb=None, nr=None, ko=None, cn=None) == _lib.E_INVALID_ARG
    assert call(kl=klass) == _lib.OK and (klass == s.klass).all()
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_sieve(frame, 16, 0.5, RAW, want_scaled=True)
        assert r.cleaned is None and r.labels is None and r.counts is None and r.n is None and r.scaled.shape == (24, 32, 3)
        for x in (out, counts, labels, n):
            x[:] = 9
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED
        assert (scaled == FramePath(c).advance_segments(frame, 1.0, RAW, want_scaled=True).scaled).all()
        assert all((x == 9).all() for x in (out, counts, labels, n))
        # a label plane that is too short: whatever infur_frame_regions answers without a model, in its own words
        want_rc = c.L.infur_frame_regions(c.h, p(frame), 64, 48, 1.0, 0, 0, 8, 16, 0, None, None, npix, p(labels), 3, None, 0, p(n), None, C.byref(ow),
                                          C.byref(oh))
        want_msg = c.last_error()
        assert call(lib=c.L, handle=c.h, lcap=3) == want_rc != _lib.OK and c.last_error() == want_msg
        assert all((x == 9).all() for x in (out, counts, labels, n))


def test_sieve_calls_leave_the_existing_legs_and_the_cached_graphs_alone(blob50):
    frames = [W.synth_frame(120, 168, index=i) for i in range(4)]
    with Context(device=0) as ce, Context(device=0, graph_replay=True) as cg:
        Model(ce).control(ModelCmd.LoadBlob(blob50))
        Model(cg).control(ModelCmd.LoadBlob(blob50))
        fe, fg = FramePath(ce), FramePath(cg)
        for it in range(10):  # past the capture
            a, _ = fe.advance(frames[it % 4], 1.0)
            b, _ = fg.advance(frames[it % 4], 1.0)
            assert (a == b).all()
        cap0, rep0, cached0 = cg.graph_stats()
        assert cap0 == 1 and cached0 == 1 and rep0 >= 1
        before = [fg.advance_regions(fr, 1.0, SOFTMAX) for fr in frames]  # the existing leg, before any Sieve call on this context
        for it in range(8):
            fr = frames[it % 4]
            kw = dict(min_pixels=64 if it & 2 else 8, factor=1.0, decode=SOFTMAX if it & 1 else RAW, connectivity=4 if it & 4 else 8, table_rows=2048)
            s, e = fg.advance_sieve(fr, **kw), fe.advance_sieve(fr, **kw)
            assert s.n == e.n and all(getattr(s, f).tobytes() == getattr(e, f).tobytes() for f in ("cleaned", "conf", "labels", "table", "counts"))
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a sieve call caused a capture"
        assert cached1 >= cached0, "a sieve call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the sieve calls were not replayed"
        for fr, b4 in zip(frames, before):  # and after: the same bytes
            now = fg.advance_regions(fr, 1.0, SOFTMAX)
            assert now.n == b4.n and all(getattr(now, f).tobytes() == getattr(b4, f).tobytes() for f in ("klass", "conf", "labels", "table"))


# --------------------------------------------------------------------------- #
# 4. composition: Sieve -> Outlines -> Coverage on klass_out
# --------------------------------------------------------------------------- #
def test_outlines_and_coverage_of_the_cleaned_plane(ctx):
    k = R.smooth(40, 70, seed=3, classes=6, cell=8)
    h, w = k.shape
    ref = sieve_reference(k, R.CONNECT_8, 64)
    loops, vertices, counts = O.outline(ref.klass_out)
    raw = O.outline(k)[2]
    assert counts[0] < raw[0] and counts[1] < raw[1]  # fewer loops and fewer vertices than the plane with its speckle
    lrows, vrows = int(counts[0]) + 3, int(counts[1]) + 3

    def outline(d):
        extra = Dev(ctx, loops=lrows * 16, vertices=vrows * 4, counts=12)
        try:
            ctx.check(ctx.L.infur_outlines_dev(ctx.h, d.ptr["klass_out"], 1, h, w, 0, 0, 0, extra.ptr["loops"], lrows, extra.ptr["vertices"], vrows,
                                               extra.ptr["counts"]))
            ctx.synchronize()
            return extra.get("loops").view(np.uint32).reshape(lrows, 4), extra.get("vertices").view(np.uint32), extra.get("counts").view(np.uint32)
        finally:
            extra.free()

    got = dev_sieve(ctx, k, R.CONNECT_8, 64, then=outline)
    gl, gv, gc = got["then"]
    assert (gc == counts).all() and (gl[:counts[0]] == loops).all() and (gv[:counts[1]] == vertices).all()
    cl, cv, cc = V.coverage(ref.klass_out, loops, vertices, counts, 16)
    dl, dv, dc = dev_coverage(ctx, got["klass_out"], gl[:counts[0]], gv[:counts[1]], gc, 16)
    assert (dc == cc).all() and (dl[:len(cl)] == cl).all() and (dv[:len(cv)] == cv).all()
    V.check_invariants(ref.klass_out, cl, cv, cc)


# --------------------------------------------------------------------------- #
# 5. the command line
# --------------------------------------------------------------------------- #
def test_cli_cleans_every_frame(tmp_path):
    import json
    import subprocess

    root = os.path.dirname(HERE)
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    (tmp_path / "clip.bgr24").write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input",
            str(tmp_path / "clip.bgr24")]
    r = subprocess.run(base + ["--labels-out", str(tmp_path / "klass.u8")], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    r = subprocess.run(base + ["--sieve", "24", "--sieve-rounds", "64", "--regions", "--connectivity", "4", "--skip-background", "--labels-out",
                               str(tmp_path / "clean.u8"), "--regions-out", str(tmp_path / "labels.u32")], capture_output=True, text=True, timeout=600,
                       cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    clean = np.frombuffer((tmp_path / "clean.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    assert len(lines) == 2
    for i in range(2):
        ref, (want_labels, _, n) = frame_reference(klass[i], 4, 24, _lib.REGIONS_SKIP_BACKGROUND, max_rounds=64)
        sv = sieve_summary(ref.counts)
        assert lines[i]["sieve"] == {k: sv[k] for k in ("small", "absorbed", "stranded", "rounds", "pixels_changed", "status")}
        assert (clean[i] == ref.klass_out).all() and (labels[i] == want_labels).all() and lines[i]["n_regions"] == n
        assert sum(c["pixels"] for c in lines[i]["classes"]) == 96 * 128
        assert {c["klass"]: c["pixels"] for c in lines[i]["classes"]} == {int(k): int(v) for k, v in zip(*np.unique(clean[i], return_counts=True))}
