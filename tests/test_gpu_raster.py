"""Raster on the device (infur_raster*, raster.hip) against tests/raster_ref.py: whole planes and counts with ==, no tolerance.

Round trips (Raster(Outlines(p)) == p, RasterRuns(Runs(p)) == p), the loops Simplify and Coverage leave (where CONFLICT and uncovered
pixels are facts of the reference, not zero), the tie rule, both forms of the edge kernel around kRasterLaneRows, overlaps, a hole
alone, a value a byte plane cannot hold, malformed runs, the guards with poisoned words behind the declared rows, rejected calls,
more loops than the grid holds waves, the device chain from Regions and from a frame's regions beside a cached frame graph, a
captured graph, a second context,
polygon_fidelity and the command line."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import compare_ref as CR  # noqa: E402
import coverage_ref as CV  # noqa: E402
import outlines_ref as O  # noqa: E402
import raster_ref as A  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as RR  # noqa: E402
import simplify_ref as S  # noqa: E402
import stage_limits as SL  # noqa: E402
import test_gpu_outlines as TO  # noqa: E402  (its poisoned, guard-padded device buffers)
from test_gpu_anchors import _hip  # noqa: E402  (the HIP runtime this process already runs on)

from infur_amd import _lib  # noqa: E402
from infur_amd.processors import (Context, FramePath, InfurError, Model, ModelCmd, Raster, RasterCmd, RasterOut, confusion_summary,  # noqa: E402
                                  polygon_fidelity)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
NONE = 0xFFFFFFFF
POISON = TO.POISON
Dev = TO.Dev
SIZES = ((1, 1), (1, 70), (23, 1), (17, 65), (64, 64), (33, 130), (3, 2100))
LANE_ROWS = SL.constant("raster.hip", "kRasterLaneRows")


@pytest.fixture(scope="module")
def ctx():
    assert _lib.load().infur_features() & _lib.FEATURE_RASTER  # (fails on a library without the feature)
    with Context(device=0) as c:
        yield c


def _fill_poisoned(d, name, arr, rows, row_bytes):
    """the array's first `rows` rows at the head of the buffer, poison behind them"""
    buf = np.full(d.sizes[name], POISON, np.uint8)
    part = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)[:rows * row_bytes]
    buf[:len(part)] = part
    d.put(name, buf)


def _outputs(d, h, w, dtype, want):
    plane = d.get("plane").view(dtype).reshape(h, w)
    counts = d.get("counts").view(np.uint32)
    for name, got in (("plane", plane), ("counts", counts)):
        if name not in want:
            assert (got.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
    return {"plane": plane if "plane" in want else None, "counts": counts if "counts" in want else None}


def dev_raster(ctx, loops, vertices, counts, h, w, dtype=np.uint8, fill=0, loops_rows_in=None, vertex_rows_in=None, want=("plane", "counts"), spare=5):
    """infur_raster_dev on poisoned device buffers -> {"plane", "counts"} as the buffers are afterwards.  The input buffers hold
    loops_rows_in records and vertex_rows_in vertices: what the arrays do not fill stays poisoned."""
    loops, vertices = np.asarray(loops, np.uint32).reshape(-1, 4), np.asarray(vertices, np.uint32)
    lin = len(loops) + spare if loops_rows_in is None else loops_rows_in
    vin = len(vertices) + spare if vertex_rows_in is None else vertex_rows_in
    d = Dev(ctx, lin=lin * 16, vin=vin * 4, cin=8, plane=h * w * np.dtype(dtype).itemsize, counts=16)
    try:
        _fill_poisoned(d, "lin", loops, lin, 16)
        _fill_poisoned(d, "vin", vertices, vin, 4)
        d.put("cin", np.asarray([int(counts[0]), int(counts[1])], np.uint32))
        before = {name: d.get(name).tobytes() for name in ("lin", "vin", "cin")}
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_raster_dev(ctx.h, d.ptr["lin"], lin, d.ptr["vin"], vin, d.ptr["cin"], h, w, np.dtype(dtype).itemsize, fill, p("plane"),
                                         p("counts")))
        ctx.synchronize()
        assert all(d.get(name).tobytes() == b for name, b in before.items())  # the input is an input
        return _outputs(d, h, w, dtype, want)
    finally:
        d.free()


def dev_raster_runs(ctx, runs, n, h, w, dtype=np.uint8, fill=0, runs_rows_in=None, want=("plane", "counts"), spare=5):
    """infur_raster_runs_dev on poisoned device buffers, as dev_raster"""
    runs = np.asarray(runs, np.uint32).reshape(-1, 3)
    rin = len(runs) + spare if runs_rows_in is None else runs_rows_in
    d = Dev(ctx, rin=rin * 12, n=4, plane=h * w * np.dtype(dtype).itemsize, counts=16)
    try:
        _fill_poisoned(d, "rin", runs, rin, 12)
        d.put("n", np.asarray([n], np.uint32))
        before = {name: d.get(name).tobytes() for name in ("rin", "n")}
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_raster_runs_dev(ctx.h, d.ptr["rin"], rin, d.ptr["n"], h, w, np.dtype(dtype).itemsize, fill, p("plane"), p("counts")))
        ctx.synchronize()
        assert all(d.get(name).tobytes() == b for name, b in before.items())
        return _outputs(d, h, w, dtype, want)
    finally:
        d.free()


def check(got, ref, name=""):
    plane, counts = ref
    assert got["counts"].tolist() == counts.tolist(), (name, got["counts"], counts)
    if plane is None:
        assert (got["plane"].view(np.uint8) == POISON).all(), (name, "truncated input wrote the plane")
    else:
        assert got["plane"].dtype == plane.dtype and (got["plane"] == plane).all(), name


def three_valued(h, w, seed, dtype=np.uint8, values=(0, 1, 2)):
    return np.asarray(values, dtype)[np.random.RandomState(seed).randint(0, len(values), size=(h, w))]


# ---------------------------------------------------------------- round trips
@functools.lru_cache(maxsize=None)
def round_trip_cases():
    """[(name, plane, flags, skip value, outline, runs)]: computed once, shared, never changed"""
    out = []
    for k, (h, w) in enumerate(SIZES):
        plane = three_valued(h, w, seed=10 + k)
        for flags in (0, O.CONN8, O.SKIP, O.SKIP | O.CONN8):
            skip = 2 if flags & O.SKIP else 0
            out.append((f"{h}x{w} flags {flags}", plane, flags, skip, O.outline(plane, flags, skip),
                        RR.encode(plane, RR.SKIP if flags & O.SKIP else 0, skip) if not flags & O.CONN8 else None))
    return out


def test_raster_of_outlines_is_the_plane(ctx):
    for name, plane, flags, skip, (l, v, c), _ in round_trip_cases():
        h, w = plane.shape
        got = dev_raster(ctx, l, v, c, h, w, np.uint8, skip if flags & O.SKIP else 77)
        assert (got["plane"] == plane).all(), name
        kept = int((plane != skip).sum()) if flags & O.SKIP else h * w
        assert got["counts"].tolist() == [int(c[0]), kept, 0, 0], name
        check(got, A.raster(l, v, c, h, w, np.uint8, skip if flags & O.SKIP else 77), name)


def test_raster_of_runs_is_the_plane(ctx):
    for name, plane, flags, skip, _, runs in round_trip_cases():
        if runs is None:
            continue
        h, w = plane.shape
        r, _, n = runs
        got = dev_raster_runs(ctx, r, n, h, w, np.uint8, skip if flags & O.SKIP else 77)
        assert (got["plane"] == plane).all(), name
        kept = int((plane != skip).sum()) if flags & O.SKIP else h * w
        assert got["counts"].tolist() == [n, kept, 0, 0], name


def test_u32_planes_with_the_largest_values(ctx):
    plane = three_valued(17, 65, seed=3, dtype=np.uint32, values=(0xFFFFFFFE, 5, NONE))
    for flags in (O.SKIP, O.SKIP | O.CONN8):
        l, v, c = O.outline(plane, flags, NONE)
        got = dev_raster(ctx, l, v, c, 17, 65, np.uint32, NONE)
        assert (got["plane"] == plane).all() and got["counts"][2] == 0
    r, _, n = RR.encode(plane, RR.SKIP, NONE)
    got = dev_raster_runs(ctx, r, n, 17, 65, np.uint32, NONE)
    assert (got["plane"] == plane).all() and got["counts"].tolist() == [n, int((plane != NONE).sum()), 0, 0]


# ---------------------------------------------------------------- behind Simplify and Coverage
@functools.lru_cache(maxsize=None)
def tolerance_cases():
    """[(name, h, w, loops, vertices, counts, reference)] for Simplify's and Coverage's reference output at four tolerances"""
    out = []
    for pname, plane, flags, skip in (("smooth", R.smooth(48, 80), 0, 0), ("stairs", S.stairs(40), O.SKIP, 0)):
        h, w = plane.shape
        l, v, c = O.outline(plane, flags, skip)
        for tol16 in (8, 16, 32, 65535):
            sl, sv, sc = S.simplify(l, v, c, w, tol16)
            out.append((f"simplify {pname} {tol16}", h, w, sl, sv, sc, A.raster(sl, sv, sc, h, w, np.uint8, 0)))
            cl, cv, cc = CV.coverage(plane, l, v, c, tol16, CV.SKIP if flags & O.SKIP else 0, skip)
            out.append((f"coverage {pname} {tol16}", h, w, cl, cv, cc, A.raster(cl, cv, cc, h, w, np.uint8, 0)))
    return out


def test_behind_simplify_and_coverage(ctx):
    seen_conflict = seen_uncovered = False
    for name, h, w, l, v, c, ref in tolerance_cases():
        check(dev_raster(ctx, l, v, c, h, w, np.uint8, 0), ref, name)
        if name.startswith("simplify smooth"):
            seen_conflict |= int(ref[1][A.CONFLICT]) > 0
            seen_uncovered |= h * w - int(ref[1][A.PAINTED]) - int(ref[1][A.CONFLICT]) > 0
    # simplified arcs of neighbouring loops cross: the reference itself says so, and the device has to agree with it above
    assert seen_conflict and seen_uncovered


# ---------------------------------------------------------------- the rule's details
def test_ties_go_to_the_right_hand_side(ctx):
    diamond = [(7, [(4, 0), (8, 4), (4, 8), (0, 4)])]
    l, v, c = A.loops_of(diamond, 8)
    got = dev_raster(ctx, l, v, c, 8, 8)
    want = A.brute(diamond, 8, 8)
    assert (got["plane"] == want[0]).all() and got["counts"].tolist() == [1, 32, 0, 0]
    assert got["plane"][0].tolist() == [0, 0, 0, 7, 0, 0, 0, 0] and got["plane"][3].tolist() == [7] * 7 + [0]
    for n in (1, 5, 9):
        tri = [(3, [(0, 0), (n, 0), (0, n)])]
        l, v, c = A.loops_of(tri, n)
        got = dev_raster(ctx, l, v, c, n, n)
        want = A.brute(tri, n, n)
        assert (got["plane"] == want[0]).all() and got["counts"].tolist() == [1, want[1], 0, 0]
        assert want[1] == n * (n - 1) // 2  # the centres on the hypotenuse lie on its left: they are not the triangle's
    # two triangles that share the diagonal with the same vertices give every pixel to exactly one of them
    n = 9
    both = [(3, [(0, 0), (n, 0), (0, n)]), (4, [(n, 0), (n, n), (0, n)])]
    l, v, c = A.loops_of(both, n)
    got = dev_raster(ctx, l, v, c, n, n)
    assert got["counts"].tolist() == [2, n * n, 0, 0] and (got["plane"] == A.brute(both, n, n)[0]).all()


def test_both_edge_forms_give_the_same_crossings(ctx):
    """segments with |dy| one below, at and one above the constant that sends a segment to the whole wave, north and south"""
    for dy in (LANE_ROWS - 1, LANE_ROWS, LANE_ROWS + 1, 64, 65, 129):
        h, w = dy + 2, 23
        poly = [(9, [(2, 1), (20, 1), (13, 1 + dy), (6, 1 + dy)])]  # both slanted sides are dy rows long
        l, v, c = A.loops_of(poly, w)
        check(dev_raster(ctx, l, v, c, h, w), A.raster(l, v, c, h, w), f"dy {dy}")
        if dy < 20:
            assert (A.raster(l, v, c, h, w)[0] == A.brute(poly, h, w)[0]).all()
    # a loop with more than 64 segments of which some are long: the ballot's bit loop beside the lane walk
    pts = [(0, 0)] + [(x, 1 + (x % 2) * (LANE_ROWS + 3)) for x in range(1, 140)] + [(140, 0)]
    l, v, c = A.loops_of([(5, pts[::-1])], 140)  # (clockwise: an outer loop)
    check(dev_raster(ctx, l, v, c, LANE_ROWS + 5, 140), A.raster(l, v, c, LANE_ROWS + 5, 140), "zigzag")


def test_long_sides(ctx):
    l, v, c = A.loops_of([(200, A.rect(0, 0, 3, 8191))], 3)
    got = dev_raster(ctx, l, v, c, 8191, 3)
    assert (got["plane"] == 200).all() and got["counts"].tolist() == [1, 3 * 8191, 0, 0]
    l, v, c = A.loops_of([(200, A.rect(0, 0, 8191, 3))], 8191)
    got = dev_raster(ctx, l, v, c, 3, 8191)
    assert (got["plane"] == 200).all() and got["counts"].tolist() == [1, 3 * 8191, 0, 0]
    slanted = [(6, [(1, 2), (60, 2), (97, 102), (38, 102)])]  # dy = 100, dx = 37
    l, v, c = A.loops_of(slanted, 100)
    check(dev_raster(ctx, l, v, c, 104, 100), A.raster(l, v, c, 104, 100), "slanted")


def test_overlap_hole_and_a_value_too_large(ctx):
    two = [(1, A.rect(1, 1, 7, 6)), (2, A.rect(4, 3, 11, 9))]
    l, v, c = A.loops_of(two, 12)
    got = dev_raster(ctx, l, v, c, 10, 12, np.uint8, 99)
    overlap = 3 * 3
    assert got["counts"].tolist() == [2, 30 + 42 - 2 * overlap, overlap, 0]
    assert (got["plane"][3:6, 4:7] == 99).all() and got["plane"][1, 1] == 1 and got["plane"][8, 10] == 2
    check(got, A.raster(l, v, c, 10, 12, np.uint8, 99))
    hole = [(1, A.rect(2, 2, 5, 4)[::-1])]  # counter-clockwise: a hole with no outer loop
    l, v, c = A.loops_of(hole, 8)
    got = dev_raster(ctx, l, v, c, 6, 8, np.uint8, 9)
    assert (got["plane"] == 9).all() and got["counts"].tolist() == [1, 0, 6, 0]
    big = [(300, A.rect(0, 0, 4, 2))]
    l, v, c = A.loops_of(big, 5)
    got = dev_raster(ctx, l, v, c, 3, 5, np.uint8, 9)
    assert (got["plane"] == 9).all() and got["counts"].tolist() == [1, 0, 8, 0]
    got = dev_raster(ctx, l, v, c, 3, 5, np.uint32, 9)
    assert (got["plane"][:2, :4] == 300).all() and got["counts"].tolist() == [1, 8, 0, 0]
    # two outer loops and a hole stacked: the winding is 1 again and the pixel reads the signed sum
    three = [(10, A.rect(0, 0, 4, 4)), (20, A.rect(1, 1, 4, 4)), (7, A.rect(2, 2, 4, 4)[::-1])]
    l, v, c = A.loops_of(three, 4)
    got = dev_raster(ctx, l, v, c, 4, 4)
    assert got["plane"][3, 3] == 23 and got["plane"][1, 1] == 0 and got["plane"][0, 0] == 10
    check(got, A.raster(l, v, c, 4, 4))


def test_runs_that_overlap_or_cross_a_row(ctx):
    h, w = 4, 10
    runs = np.array([[2, 8, 5], [5, 9, 6], [12, 23, 7], [30, 40, 8], [35, 35, 1], [38, 41, 2], [20, 30, 3]], np.uint32)
    got = dev_raster_runs(ctx, runs, len(runs), h, w, np.uint8, 0)
    ref = A.raster_runs(runs, len(runs), h, w)
    check(got, ref)
    assert got["counts"].tolist() == [7, 3 + 1 + 10 + 10, 3, _lib.RASTER_MALFORMED]
    assert got["plane"][0].tolist() == [0, 0, 5, 5, 5, 0, 0, 0, 6, 0] and (got["plane"][1] == 0).all()


# ---------------------------------------------------------------- guards
def test_truncated_malformed_and_outside(ctx):
    plane = R.smooth(20, 31, seed=2, classes=4, cell=5)
    l, v, c = O.outline(plane, O.CONN8)
    h, w = plane.shape
    # truncated either way: only the counts are written, whatever the poisoned words behind the rows say
    for kw in (dict(loops_rows_in=len(l) - 1), dict(vertex_rows_in=len(v) - 1)):
        got = dev_raster(ctx, l, v, c, h, w, **kw)
        check(got, A.raster(l, v, c, h, w, **kw), str(kw))
        assert got["counts"].tolist() == [len(l), 0, 0, _lib.RASTER_TRUNCATED]
    # rows that are exactly enough: nothing behind them is read
    check(dev_raster(ctx, l, v, c, h, w, loops_rows_in=len(l), vertex_rows_in=len(v)), (plane, np.array([len(l), h * w, 0, 0], np.uint32)))
    # malformed records are skipped: a COUNT below 2, vertices that end beyond the count, an OFFSET near 2^32
    bad = l.copy()
    bad[1, 1] = 1
    bad[3, 0] = len(v) - 1
    bad[5, 0] = 0xFFFFFFFF
    got = dev_raster(ctx, bad, v, c, h, w)
    ref = A.raster(bad, v, c, h, w)
    check(got, ref, "malformed")
    assert ref[1][A.STATUS] == _lib.RASTER_MALFORMED
    # vertex ids beyond the lattice are clamped onto it
    far = v.copy()
    far[2] = NONE
    far[7] = (h + 3) * (w + 1) + 4
    got = dev_raster(ctx, l, far, c, h, w)
    ref = A.raster(l, far, c, h, w)
    check(got, ref, "outside")
    assert ref[1][A.STATUS] & _lib.RASTER_OUTSIDE
    # runs: a count above the rows, and records beyond the plane
    r, _, n = RR.encode(plane)
    got = dev_raster_runs(ctx, r, n, h, w, runs_rows_in=n - 1)
    assert got["counts"].tolist() == [n, 0, 0, _lib.RASTER_TRUNCATED] and (got["plane"].view(np.uint8) == POISON).all()
    wild = np.array([[0, 5, 1], [h * w - 2, h * w + 1, 2], [NONE - 1, NONE, 3], [7, 3, 4]], np.uint32)
    check(dev_raster_runs(ctx, wild, 4, h, w), A.raster_runs(wild, 4, h, w), "wild runs")


def test_each_output_alone(ctx):
    plane = three_valued(9, 70, seed=1)
    l, v, c = O.outline(plane)
    ref = A.raster(l, v, c, 9, 70)
    got = dev_raster(ctx, l, v, c, 9, 70, want=("plane",))
    assert (got["plane"] == plane).all()
    got = dev_raster(ctx, l, v, c, 9, 70, want=("counts",))
    assert got["counts"].tolist() == ref[1].tolist()
    r, _, n = RR.encode(plane)
    assert (dev_raster_runs(ctx, r, n, 9, 70, want=("plane",))["plane"] == plane).all()
    assert dev_raster_runs(ctx, r, n, 9, 70, want=("counts",))["counts"].tolist() == [n, 630, 0, 0]


def test_rejected_calls_touch_nothing(ctx):
    L = ctx.L
    d = Dev(ctx, lin=64, vin=64, cin=8, plane=64, counts=16)
    try:
        d.put("cin", np.array([0, 0], np.uint32))
        p = d.ptr
        calls = [
            lambda: L.infur_raster_dev(ctx.h, p["lin"], 1, p["vin"], 4, p["cin"], 4, 4, 2, 0, p["plane"], p["counts"]),  # elem_bytes
            lambda: L.infur_raster_dev(ctx.h, p["lin"], 1, p["vin"], 4, p["cin"], 4, 4, 1, 256, p["plane"], p["counts"]),  # fill on bytes
            lambda: L.infur_raster_dev(ctx.h, p["lin"], 1, p["vin"], 4, p["cin"], 0, 4, 1, 0, p["plane"], p["counts"]),  # no rows
            lambda: L.infur_raster_dev(ctx.h, p["lin"], 1, p["vin"], 4, p["cin"], 4, 8192, 1, 0, p["plane"], p["counts"]),  # too wide
            lambda: L.infur_raster_dev(ctx.h, p["lin"], 1, p["vin"], 4, p["cin"], 4, 4, 1, 0, None, None),  # nothing wanted
            lambda: L.infur_raster_dev(ctx.h, p["lin"], 1, p["vin"], 4, None, 4, 4, 1, 0, p["plane"], p["counts"]),  # no counts
            lambda: L.infur_raster_dev(ctx.h, None, 1, p["vin"], 4, p["cin"], 4, 4, 1, 0, p["plane"], p["counts"]),  # rows and no pointer
            lambda: L.infur_raster_runs_dev(ctx.h, p["lin"], 1, None, 4, 4, 1, 0, p["plane"], p["counts"]),  # no count
            lambda: L.infur_raster_runs_dev(ctx.h, None, 1, p["cin"], 4, 4, 1, 0, p["plane"], p["counts"]),
            lambda: L.infur_raster_runs_dev(ctx.h, p["lin"], 1, p["cin"], 4, 4, 4, 0, None, None),
            lambda: L.infur_raster_runs_dev(ctx.h, p["lin"], 1, p["cin"], 8192, 4, 4, 0, p["plane"], p["counts"]),
        ]
        for k, call in enumerate(calls):
            assert call() == _lib.E_INVALID_ARG, k
        ctx.synchronize()
        assert (d.get("plane") == POISON).all() and (d.get("counts") == POISON).all()
        host = np.full(16, POISON, np.uint8)
        cout = np.full(4, TO.POISON32, np.uint32)
        cin = np.zeros(2, np.uint32)
        assert L.infur_raster(ctx.h, None, 0, None, 0, cin.ctypes.data, 4, 4, 1, 300, host.ctypes.data, cout.ctypes.data) == _lib.E_INVALID_ARG
        assert L.infur_raster_runs(ctx.h, None, 0, 0, 4, 0, 1, 0, host.ctypes.data, cout.ctypes.data) == _lib.E_INVALID_ARG
        assert (host == POISON).all() and (cout == TO.POISON32).all()
        assert "fill_value" in ctx.last_error() or "plane of width" in ctx.last_error()
    finally:
        d.free()


def test_more_loops_than_the_grid_holds_waves(ctx):
    """one pixel square at every other pixel: more loops than kLoopGrid workgroups have waves, so waves meet a second loop"""
    waves = SL.constant("raster.hip", "kLoopGrid") * (SL.constant("raster.hip", "kLoopBlock") // 64)
    h, w = 182, 724
    ys, xs = np.meshgrid(np.arange(0, h, 2), np.arange(0, w, 2), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    n = len(ys)
    assert n > waves
    values = (np.arange(n) % 251 + 1).astype(np.uint32)
    w1 = w + 1
    vertices = np.stack([ys * w1 + xs, ys * w1 + xs + 1, (ys + 1) * w1 + xs + 1, (ys + 1) * w1 + xs], axis=1).astype(np.uint32).reshape(-1)
    loops = np.stack([np.arange(n) * 4, np.full(n, 4), values, np.zeros(n)], axis=1).astype(np.uint32)
    want = np.zeros((h, w), np.uint8)
    want[ys, xs] = values
    got = dev_raster(ctx, loops, vertices, (n, 4 * n), h, w)
    assert (got["plane"] == want).all() and got["counts"].tolist() == [n, n, 0, 0]


# ---------------------------------------------------------------- composition
def test_host_calls_and_the_processor(ctx):
    plane = three_valued(33, 130, seed=8)
    l, v, c = O.outline(plane, O.SKIP, 0)
    r = Raster(ctx, np.uint8, 0)
    assert r.is_dirty()
    out = RasterOut()
    r.advance((l, v, c, plane.shape), out)
    assert not r.is_dirty() and (out.plane == plane).all() and (out.n, out.painted, out.conflict, out.status) == (len(l), int((plane != 0).sum()), 0, 0)
    runs, _, n = RR.encode(plane, RR.SKIP, 0)
    r.advance((runs, n, plane.shape), out)
    assert (out.plane == plane).all() and out.n == n
    r.advance((l, v, (len(l) + 1, len(v)), plane.shape), out)
    assert out.plane is None and out.status == _lib.RASTER_TRUNCATED
    r.control(RasterCmd(np.uint32, NONE))
    assert r.is_dirty()
    r.advance((l, v, c, plane.shape), out)
    assert out.plane.dtype == np.uint32 and (out.plane == np.where(plane == 0, NONE, plane.astype(np.uint32))).all()
    with pytest.raises(InfurError):
        r.control(RasterCmd(np.uint8, 256))
    out = RasterOut(want_plane=False)
    r.advance((l, v, c, plane.shape), out)
    assert out.plane is None and out.painted == int((plane != 0).sum())


def test_outlines_dev_then_raster_dev_is_the_label_plane(ctx):
    """the loops never leave the device: infur_regions_dev -> infur_outlines_dev -> infur_raster_dev equals the label plane"""
    klass = R.smooth(40, 70, seed=3, classes=5, cell=9)
    h, w = klass.shape
    labels, _, n = R.label(klass, connectivity=R.CONNECT_8, flags=R.SKIP_BACKGROUND)
    d = Dev(ctx, klass=h * w, labels=h * w * 4, n=4, loops=h * w * 16, vertices=4 * h * w * 4, counts=12, plane=h * w * 4, rcounts=16)
    try:
        d.put("klass", klass)
        L = ctx.L
        ctx.check(L.infur_regions_dev(ctx.h, d.ptr["klass"], None, h, w, _lib.CONNECT_8, 0, _lib.REGIONS_SKIP_BACKGROUND, d.ptr["labels"], None, 0,
                                      d.ptr["n"]))
        ctx.check(L.infur_outlines_dev(ctx.h, d.ptr["labels"], 4, h, w, _lib.OUTLINES_SKIP | _lib.OUTLINES_CONN8, NONE, 0, d.ptr["loops"], h * w,
                                       d.ptr["vertices"], 4 * h * w, d.ptr["counts"]))
        ctx.check(L.infur_raster_dev(ctx.h, d.ptr["loops"], h * w, d.ptr["vertices"], 4 * h * w, d.ptr["counts"], h, w, 4, NONE, d.ptr["plane"],
                                     d.ptr["rcounts"]))
        ctx.synchronize()
        got = d.get("plane").view(np.uint32).reshape(h, w)
        assert (got == labels).all() and (got == d.get("labels").view(np.uint32).reshape(h, w)).all()
        rc = d.get("rcounts").view(np.uint32)
        assert rc[1] == int((labels != NONE).sum()) and rc[2] == 0 and rc[3] == 0
    finally:
        d.free()


def test_frame_regions_dev_then_outlines_dev_then_raster_dev_is_the_label_plane(blob50):
    """infur_frame_regions_dev -> infur_outlines_dev -> infur_raster_dev in a context with a loaded model and a cached frame graph:
    the plane equals the label plane the frame call left and FramePath.advance_regions', and the stage's scratch, first made for
    a 4 x 4 plane and then grown for the frame's, causes no capture and drops no cached graph.  (The caller's buffers are
    allocated before the graph is captured: every infur_dev_alloc moves the generation the cached graphs are checked against.)"""
    from infur_amd import weights as W

    frames = [W.synth_frame(96, 128, index=i) for i in range(3)]
    hh, ww = 96, 128
    with Context(device=0, graph_replay=True) as c:
        Model(c).control(ModelCmd.LoadBlob(blob50))
        fp, L = FramePath(c), c.L
        d = Dev(c, bgr=frames[0].nbytes, labels=hh * ww * 4, n=4, loops=hh * ww * 16, vertices=4 * hh * ww * 4, counts=12, plane=hh * ww * 4, rcounts=16,
                zero=8, small=16)
        try:
            P = d.ptr
            d.put("zero", np.zeros(2, np.uint32))
            for it in range(10):  # past the capture
                first, _ = fp.advance(frames[it % 3], 1.0)
            cap0, rep0, cached0 = c.graph_stats()
            assert cap0 == 1 and cached0 == 1 and rep0 >= 1
            c.check(L.infur_raster_dev(c.h, None, 0, None, 0, P["zero"], 4, 4, 1, 7, P["small"], None))  # the scratch of a 4 x 4 plane
            for k, conn in enumerate((4, 8)):
                frame = frames[1 + k]
                r = fp.advance_regions(frame, 1.0, _lib.DECODE_SOFTMAX, connectivity=conn, min_pixels=20, flags=_lib.REGIONS_SKIP_BACKGROUND, table_rows=512)
                assert r.labels.shape == (hh, ww) and r.n > 1 and (r.labels == NONE).any()
                d.put("bgr", frame)
                d.poison("plane", "rcounts")
                ow, oh = C.c_uint32(0), C.c_uint32(0)
                c.check(L.infur_frame_regions_dev(c.h, P["bgr"], ww, hh, 1.0, 0, _lib.DECODE_SOFTMAX, conn, 20, _lib.REGIONS_SKIP_BACKGROUND, None, None, 0,
                                                  P["labels"], hh * ww * 4, None, 0, P["n"], None, C.byref(ow), C.byref(oh)))
                assert (oh.value, ow.value) == (hh, ww)
                c.check(L.infur_outlines_dev(c.h, P["labels"], 4, hh, ww, _lib.OUTLINES_SKIP | (_lib.OUTLINES_CONN8 if conn == 8 else 0), NONE, 0, P["loops"],
                                             hh * ww, P["vertices"], 4 * hh * ww, P["counts"]))
                c.check(L.infur_raster_dev(c.h, P["loops"], hh * ww, P["vertices"], 4 * hh * ww, P["counts"], hh, ww, 4, NONE, P["plane"], P["rcounts"]))
                c.synchronize()
                got = d.get("plane").view(np.uint32).reshape(hh, ww)
                assert (got == d.get("labels").view(np.uint32).reshape(hh, ww)).all() and (got == r.labels).all(), k
                assert d.get("rcounts").view(np.uint32)[1:].tolist() == [int((r.labels != NONE).sum()), 0, 0], k
                again, _ = fp.advance(frames[0], 1.0)  # the cached graph still replays, to the same bytes
                assert (again == first).all()  # (iteration 9 of the warm-up was frames[0] too)
            assert (d.get("small") == 7).all()
            cap1, rep1, cached1 = c.graph_stats()
            assert cap1 == cap0, "a raster call caused a capture"
            assert cached1 >= cached0, "a raster call dropped a cached graph"
            assert rep1 == rep0 + 2, "the frames between the raster calls were not replayed"
        finally:
            d.free()


def test_inside_a_captured_graph_and_in_a_second_context(ctx):
    hip = _hip()
    plane = three_valued(17, 65, seed=4)
    l, v, c = O.outline(plane, O.CONN8)
    h, w = plane.shape
    with Context(device=0) as c2:
        d = Dev(c2, lin=len(l) * 16, vin=len(v) * 4, cin=8, plane=h * w, counts=16)
        try:
            d.put("lin", l)
            d.put("vin", v)
            d.put("cin", np.asarray(c[:2], np.uint32))
            call = lambda: c2.check(c2.L.infur_raster_dev(c2.h, d.ptr["lin"], len(l), d.ptr["vin"], len(v), d.ptr["cin"], h, w, 1, 0,  # noqa: E731
                                                          d.ptr["plane"], d.ptr["counts"]))
            call()  # outside the capture: allocates the scratch
            c2.synchronize()
            assert (d.get("plane").reshape(h, w) == plane).all()
            stream = C.c_void_p(c2.stream)
            graph, inst = C.c_void_p(None), C.c_void_p(None)
            assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
            call()
            assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
            assert hip.hipGraphInstantiate(C.byref(inst), graph, None, None, 0) == 0
            for _ in range(2):
                d.poison("plane", "counts")
                assert hip.hipGraphLaunch(inst, stream) == 0
                c2.synchronize()
                assert (d.get("plane").reshape(h, w) == plane).all()
                assert d.get("counts").view(np.uint32).tolist() == [len(l), h * w, 0, 0]
            assert hip.hipGraphExecDestroy(inst) == 0 and hip.hipGraphDestroy(graph) == 0
        finally:
            d.free()
    # the first context is untouched by the second
    assert (dev_raster(ctx, l, v, c, h, w)["plane"] == plane).all()


# ---------------------------------------------------------------- polygon_fidelity and the command line
def fidelity_ref(plane, tol16, shared, flags, skip, rows):
    h, w = plane.shape
    l, v, c = O.outline(plane, flags, skip or 0)
    if shared:
        l2, v2, c2 = CV.coverage(plane, l, v, c, tol16, CV.SKIP if flags & O.SKIP else 0, skip or 0)
    else:
        l2, v2, c2 = S.simplify(l, v, c, w, tol16)
    fill = skip if skip is not None else 255
    filled, rc = A.raster(l2, v2, c2, h, w, plane.dtype, fill)
    res = CR.compare(plane, filled, 0, 0, 0, rows, rows)
    s = confusion_summary(res.matrix, names=lambda k: None)
    skipped = int((plane == skip).sum()) if skip is not None else 0
    return {"vertices_in": int(c[1]), "vertices_out": int(c2[1]), "changed": int((filled != plane).sum()), "conflict": int(rc[A.CONFLICT]),
            "uncovered": h * w - int(rc[A.PAINTED]) - int(rc[A.CONFLICT]) - skipped, "status": int(rc[A.STATUS]),
            "pixel_accuracy": s["pixel_accuracy"], "miou": s["miou"]}


def test_polygon_fidelity_is_the_chain_of_the_references(ctx):
    plane = R.smooth(48, 80)
    for tol16, shared, conn, skip in ((16, False, 4, None), (16, True, 4, None), (32, True, 8, None), (8, False, 8, 0), (0, False, 4, None)):
        flags = (O.SKIP if skip is not None else 0) | (O.CONN8 if conn == 8 else 0)
        got = polygon_fidelity(ctx, plane, tol16, shared=shared, connectivity=conn, skip=skip, rows=21)
        assert got == fidelity_ref(plane, tol16, shared, flags, skip, 21), (tol16, shared, conn, skip)
    exact = polygon_fidelity(ctx, plane, 0, rows=21)
    assert exact["changed"] == exact["conflict"] == exact["uncovered"] == 0 and exact["pixel_accuracy"] == 1.0


def test_cli_says_what_the_tolerance_costs(tmp_path):
    from infur_amd import weights as W  # (the synthetic frames of the other command-line tests)

    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    cmd = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip),
           "--labels-out", str(tmp_path / "klass.u8"), "--outlines-tolerance", "1", "--outlines-shared", "--outlines-fidelity"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    assert len(lines) == 3
    total = {k: 0 for k in ("vertices_in", "vertices_out", "changed", "conflict", "uncovered")}
    for i in range(2):
        want = fidelity_ref(klass[i], 16, True, O.CONN8, None, 21)  # (8-connectivity is the command line's default)
        assert lines[i]["polygon_fidelity"] == want, i
        for k in total:
            total[k] += want[k]
    assert lines[2] == {"frames": 2, "polygon_fidelity": total}
    bad = subprocess.run(cmd[:-4] + ["--outlines-fidelity"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert bad.returncode != 0 and "--outlines-fidelity needs --outlines-tolerance" in bad.stderr
