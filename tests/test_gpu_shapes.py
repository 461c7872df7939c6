"""Shapes on the GPU: hull records, hull vertices, per-loop records, per-value rows and counts of ``infur_shapes*`` and of the fused
``infur_frame_shapes*`` against tests/shapes_ref.py.  Every quantity is an exact integer function of a loop, so every comparison
is ``==`` on whole arrays.  Every output buffer is filled with a poison byte first and has guard bytes behind it: what a call must
leave alone still holds the poison afterwards, and what it must write owes nothing to an initialisation."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd, Outlines, OutlinesOut, Shapes, ShapesOut, outlines_polygons, shape_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import shapes_ref as H  # noqa: E402
import simplify_ref as S  # noqa: E402
import test_gpu_outlines as TO  # noqa: E402  (its poisoned, guard-padded device buffers and its families)
from test_gpu_anchors import _hip  # noqa: E402  (the HIP runtime this process already runs on)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
SKIP, CONN8 = _lib.OUTLINES_SKIP, _lib.OUTLINES_CONN8
NONE = 0xFFFFFFFF
POISON, POISON32 = TO.POISON, TO.POISON32
Dev = TO.Dev
OUTPUTS = ("loops", "vertices", "shapes", "values", "counts")
SIZES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (135, 241), (300, 3))
ROWS = 24  # per-value rows of the family tests: above the 21 classes, below most u32 values


def planes():
    """(name, u8 plane): the families of regions_ref at the nine sizes -- at 135 x 241 the three that have long loops -- and the
    disc of 243 x 243, an annulus, the C and the bar"""
    for h, w in SIZES:
        for name, k in TO.families(h, w):
            if h * w > 20000 and name not in ("smooth", "noise2", "staircase"):
                continue
            yield f"{name} {h}x{w}", k
    yield "spiral 33x63", R.spiral(33, 63)
    yield "serpentine 40x70", R.serpentine(40, 70)
    yield "disc 243x243", H.disc(120)
    yield "annulus 43x43", H.annulus(20, 9)
    yield "c 24x24", H.letter_c()
    yield "bar 12x16", H.bar()


@functools.lru_cache(maxsize=None)
def plane_cases(elem_bytes, flags):
    """[(name, plane, outline, reference)]: computed once, shared, never changed.  With SKIP value 0 belongs to no region"""
    out = []
    for name, k in planes():
        plane = TO.as_elem(k, elem_bytes)
        o = O.outline(plane, flags, 0)
        out.append((name, plane, o, H.shapes(*o, plane.shape[1], rows=ROWS)))
    return out


def dev_shapes(ctx, loops, vertices, counts, h, w, rows=ROWS, loops_rows_in=None, vertex_rows_in=None, loops_rows_out=None, vertex_rows_out=None,
               shape_rows=None, want=OUTPUTS, spare=5):
    """infur_shapes_dev on poisoned device buffers -> {name: the buffer as it is afterwards}, None for what was not wanted (and that
    buffer is checked to be untouched).  The input buffers hold loops_rows_in records and vertex_rows_in vertices: what the arrays
    do not fill stays poisoned."""
    loops, vertices = np.asarray(loops, np.uint32).reshape(-1, 4), np.asarray(vertices, np.uint32)
    lin = len(loops) + spare if loops_rows_in is None else loops_rows_in
    vin = len(vertices) + spare if vertex_rows_in is None else vertex_rows_in
    lout = len(loops) + spare if loops_rows_out is None else loops_rows_out
    vout = len(vertices) + spare if vertex_rows_out is None else vertex_rows_out
    srows = len(loops) + spare if shape_rows is None else shape_rows
    d = Dev(ctx, lin=lin * 16, vin=vin * 4, cin=12, loops=lout * 16, vertices=vout * 4, shapes=srows * 96, values=rows * 96, counts=16)
    try:
        for name, arr, n in (("lin", loops, lin), ("vin", vertices, vin)):
            buf = np.full(d.sizes[name], POISON, np.uint8)
            part = arr[:n].reshape(-1).view(np.uint8)
            buf[:len(part)] = part
            d.put(name, buf)
        d.put("cin", np.asarray(list(counts)[:3] + [0] * (3 - min(3, len(counts))), np.uint32))
        before = {name: d.get(name).tobytes() for name in ("lin", "vin", "cin")}
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_shapes_dev(ctx.h, d.ptr["lin"], lin, d.ptr["vin"], vin, d.ptr["cin"], h, w, p("loops"), lout, p("vertices"), vout,
                                         p("shapes"), srows, p("values"), rows, p("counts")))
        ctx.synchronize()
        got = {"loops": d.get("loops").view(np.uint32).reshape(lout, 4), "vertices": d.get("vertices").view(np.uint32),
               "shapes": d.get("shapes").view(np.int64).reshape(srows, 12), "values": d.get("values").view(np.int64).reshape(rows, 12),
               "counts": d.get("counts").view(np.uint32)}
        assert all(d.get(name).tobytes() == b for name, b in before.items())  # the input is an input
        for name in OUTPUTS:
            if name not in want:
                assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
                got[name] = None
        return got
    finally:
        d.free()


def check_result(ref, got, name=""):
    """whole arrays against the reference's; what lies behind the counts still holds the poison"""
    rl, rv, rs, rvals, rc = ref
    assert got["counts"].tolist() == rc.tolist(), (name, got["counts"], rc)
    for key, want in (("loops", rl), ("vertices", rv), ("shapes", rs)):
        g = got[key]
        n = min(len(want), len(g))
        assert (g[:n] == want[:n]).all(), (name, key)
        assert (g[n:].view(np.uint8) == POISON).all(), (name, key)
    assert (got["values"] == rvals[:len(got["values"])]).all(), (name, "values")


# --------------------------------------------------------------------------- #
# 1. from planes: Outlines -> Shapes on the device
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conn", [0, CONN8])
@pytest.mark.parametrize("skip", [0, SKIP])
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_planes_through_outlines_on_the_device(ctx, elem_bytes, skip, conn):
    assert ctx.L.infur_features() & _lib.FEATURE_SHAPES  # (the first line: fails on a library without the feature)
    loops = hull = 0
    for name, plane, (l, v, c), ref in plane_cases(elem_bytes, skip | conn):
        h, w = plane.shape
        lrows, vrows = len(l) + 3, len(v) + 3
        d = Dev(ctx, plane=plane.nbytes, lin=lrows * 16, vin=vrows * 4, cin=12, loops=lrows * 16, vertices=vrows * 4, shapes=lrows * 96,
                values=ROWS * 96, counts=16)
        try:
            d.put("plane", plane)
            P = d.ptr
            ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["plane"], elem_bytes, h, w, skip | conn, 0, 0, P["lin"], lrows, P["vin"], vrows, P["cin"]))
            ctx.check(ctx.L.infur_shapes_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], h, w, P["loops"], lrows, P["vertices"], vrows,
                                             P["shapes"], lrows, P["values"], ROWS, P["counts"]))
            ctx.synchronize()
            got = {"loops": d.get("loops").view(np.uint32).reshape(-1, 4), "vertices": d.get("vertices").view(np.uint32),
                   "shapes": d.get("shapes").view(np.int64).reshape(-1, 12), "values": d.get("values").view(np.int64).reshape(-1, 12),
                   "counts": d.get("counts").view(np.uint32)}
            check_result(ref, got, name)
            assert d.get("cin").view(np.uint32).tolist() == c.tolist() and (d.get("lin").view(np.uint32).reshape(-1, 4)[:len(l)] == l).all()
        finally:
            d.free()
        loops += int(c[0])
        hull += int(ref[4][1])
    print(f"elem {elem_bytes} skip {skip} conn {conn}: {loops} loops, {hull} hull vertices")
    assert loops > 5000


def test_the_pinned_facts(ctx):
    """the worked examples and the disc table of the issue, from the device"""
    for plane, record, hull in ((H.letter_c(), [500, 110, 15750, 18000, 439000, 577000, 756000, 800, 0, 400, 400, 400], [(2, 2), (22, 2), (22, 22), (2, 22)]),
                                (H.bar(), [60, 44, 1440, 1080, 26280, 15960, 40500, 78, 1, 198, 36, 162], [(2, 1), (5, 1), (14, 10), (14, 11), (11, 11), (2, 2)])):
        h, w = plane.shape
        got = dev_shapes(ctx, *O.outline(plane, SKIP, 0), h, w, rows=3)
        assert got["shapes"][0].tolist() == record and got["counts"].tolist() == [1, len(hull), 0, len(hull)]
        assert list(zip(*S._xy(got["vertices"][:len(hull)], w))) == hull
        assert got["values"][int(plane.max()), :8].tolist() == record[:8] and got["values"][int(plane.max()), 8:].tolist() == [1, 0, 0, 0]
    for r, n, k, rect in ((10, 52, 24, [1, 85, 85, 17]), (40, 196, 48, [1, 649, 649, 65]), (120, 572, 88, [11, 5100, 5100, 450])):
        plane = H.disc(r)
        l, v, c = O.outline(plane, SKIP, 0)
        got = dev_shapes(ctx, l, v, c, *plane.shape, rows=2)
        assert c[1] == n and got["counts"].tolist() == [1, k, 0, k] and got["shapes"][0, 8:].tolist() == rect  # k = 88: the rectangle's second stride


# --------------------------------------------------------------------------- #
# 2. from hand-made loops, no plane
# --------------------------------------------------------------------------- #
def test_hand_made_loops(ctx):
    side = 8191
    l, v, c = H.loop_of([(0, 0), (side, 0), (side, side), (0, side)], side)
    ref = H.shapes(l, v, c, side, rows=2)
    assert ref[2][0, H.M20_12] == 4 * side ** 4  # the largest magnitude
    check_result(ref, dev_shapes(ctx, l, v, c, side, side, rows=2), "square")
    l, v, c = H.loop_of(H.diagonal_staircase(8000), side)  # 16,002 vertices: the lanes' sums wrap on the way, the result fits
    check_result(H.shapes(l, v, c, side, rows=2), dev_shapes(ctx, l, v, c, side, side, rows=2), "diagonal")
    for kk in (3, 30, 31, 32, 63, 64, 100):
        l, v, c = O.outline(S.stairs(kk), SKIP, 0)
        check_result(H.shapes(l, v, c, kk, rows=2), dev_shapes(ctx, l, v, c, kk, kk, rows=2), ("stairs", kk))
    comb = S.comb(130, 2100)  # one loop of more than 2^16 vertices: lopsided recursion, many strides
    l, v, c = O.outline(comb, SKIP, 0)
    assert c[0] == 1 and c[1] > 1 << 16
    check_result(H.shapes(l, v, c, 2100, rows=2), dev_shapes(ctx, l, v, c, 130, 2100, rows=2), "comb")
    for n in (4, 63, 64, 65, 129):
        pts = H.polygon_of(n)
        for turn in (0, 1, n // 2, n - 1):
            for seq in (pts[turn:] + pts[:turn], (pts[turn:] + pts[:turn])[::-1]):
                l, v, c = H.loop_of(seq, 80)
                check_result(H.shapes(l, v, c, 80, rows=2), dev_shapes(ctx, l, v, c, 70, 80, rows=2), ("polygon", n, turn))
    # a loop that is one point, and one that is a segment: COUNT' 1 and 2, a rectangle of zeros and of no height
    l, v, c = H.loop_of([(3, 4)] * 70 + [(1, 1), (9, 5)], 12)
    l = np.array([[0, 70, 1, 0], [70, 2, 1, 4]], np.uint32)
    c = np.array([2, 72, 0], np.uint32)
    ref = H.shapes(l, v, c, 12, rows=2)
    assert ref[0][:, 1].tolist() == [1, 2] and ref[2][0].tolist() == [0] * 12 and ref[2][1, 7:].tolist() == [0, 0, 80, 0, 80]
    check_result(ref, dev_shapes(ctx, l, v, c, 7, 12, rows=2), "degenerate")


# --------------------------------------------------------------------------- #
# 3. arguments
# --------------------------------------------------------------------------- #
def smooth_case():
    k = R.smooth(65, 130)
    l, v, c = O.outline(k)
    return k, (l, v, c), H.shapes(l, v, c, 130, rows=ROWS)


def test_rows_of_the_per_value_table(ctx):
    k, (l, v, c), _ = smooth_case()
    values = int(k.max()) + 1
    for rows in (0, 1, values - 1, values, values + 5):
        got = dev_shapes(ctx, l, v, c, 65, 130, rows=rows)
        check_result(H.shapes(l, v, c, 130, rows=rows), got, rows)  # every row written, none behind them (the guard)
    got = dev_shapes(ctx, l, v, c, 65, 130, rows=values + 5)
    assert (got["values"][values:, :10] == 0).all() and (got["values"][values:, H.LOOP] == -1).all()


def test_every_subset_of_the_outputs(ctx):
    k, (l, v, c), ref = smooth_case()
    for mask in range(1, 32):
        want = tuple(name for i, name in enumerate(OUTPUTS) if mask >> i & 1)
        got = dev_shapes(ctx, l, v, c, 65, 130, want=want, spare=0)
        for name, r in zip(OUTPUTS, ref):
            assert got[name] is None or (got[name][:len(r)] == r).all(), (want, name)
    # pointers with no rows are no tables
    got = dev_shapes(ctx, l, v, c, 65, 130, rows=0, loops_rows_out=0, vertex_rows_out=0, shape_rows=0)
    assert got["counts"].tolist() == ref[4].tolist()


def test_short_and_ample_output_rows(ctx):
    k, (l, v, c), ref = smooth_case()
    nl, nv = len(ref[0]), len(ref[1])
    assert nl > 8 and nv > 8
    for lrows, vrows, srows in ((0, nv, nl), (1, nv, 1), (nl - 1, nv, nl + 7), (nl, nv, 0), (nl + 7, nv, nl - 1), (nl, 0, nl), (nl, 1, nl), (nl, nv - 1, nl),
                                (nl, nv + 7, nl), (1, 1, 1)):
        got = dev_shapes(ctx, l, v, c, 65, 130, loops_rows_out=lrows, vertex_rows_out=vrows, shape_rows=srows)
        check_result(ref, got, (lrows, vrows, srows))  # the full counts and prefix sums: that is how a caller sees truncation


def test_truncated_and_malformed_input(ctx):
    """the lane emulation first (tests/test_shapes_cpu.py runs the same inputs); on the device they stay inside the guards"""
    k, (l, v, c), good = smooth_case()
    nl, nv = len(l), len(v)
    for lin, vin in ((nl - 1, nv), (nl, nv - 1), (1, 1), (0, nv), (nl, 0), (0, 0)):
        emu = H.emulate(l, v, c, 130, rows=4, loops_rows_in=lin, vertex_rows_in=vin, loops_rows_out=nl, vertex_rows_out=nv, shape_rows=nl)
        got = dev_shapes(ctx, l, v, c, 65, 130, rows=4, loops_rows_in=lin, vertex_rows_in=vin, loops_rows_out=nl, vertex_rows_out=nv, shape_rows=nl)
        assert got["counts"].tolist() == emu[4].tolist() == [nl, 0, _lib.SHAPES_TRUNCATED, 0], (lin, vin)
        assert all((got[name].view(np.uint8) == POISON).all() for name in ("loops", "vertices", "shapes")), (lin, vin)
        assert (got["values"] == emu[3]).all() and (got["values"][:, H.LOOP] == -1).all() and (got["values"][:, :10] == 0).all()
    assert dev_shapes(ctx, l, v, c, 65, 130, loops_rows_in=nl, vertex_rows_in=nv)["counts"][2] == 0  # rows as large as the counts: not truncated
    # no record here points outside the vertices the test itself allocated: the bad ranges end inside the spare rows
    bad = l.copy()
    bad[2, 1] = 1
    bad[5, 1] = 0
    bad[nl - 1, 1] += 3
    bad[nl - 3, 0], bad[nl - 3, 1] = nv + 9, 4
    ref = H.shapes(bad, v, c, 130, rows=ROWS)
    assert ref[4][2] == _lib.SHAPES_MALFORMED and same_arrays(H.emulate(bad, v, c, 130, rows=ROWS), ref)
    check_result(ref, dev_shapes(ctx, bad, v, c, 65, 130, spare=64), "malformed")
    keep = np.ones(nl, bool)
    keep[[2, 5, nl - 1, nl - 3]] = False
    assert (ref[2][keep] == good[2][keep]).all()


def same_arrays(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    k, (l, v, c), ref = smooth_case()
    d = Dev(ctx, lin=l.nbytes, vin=v.nbytes, cin=12, loops=l.nbytes, vertices=v.nbytes, shapes=len(l) * 96, values=ROWS * 96, counts=16)
    try:
        d.put("lin", l)
        d.put("vin", v)
        d.put("cin", c)
        P = d.ptr
        call = lambda hh=65, ww=130, li=P["lin"], ve=P["vin"], n=P["cin"], lo=P["loops"], vo=P["vertices"], sh=P["shapes"], va=P["values"], co=P["counts"]: L.infur_shapes_dev(  # noqa: E731
            h, li, len(l), ve, len(v), n, hh, ww, lo, len(l), vo, len(v), sh, len(l), va, ROWS, co)
        assert call(ww=0) == _lib.E_INVALID_ARG and call(ww=8192) == _lib.E_INVALID_ARG and call(ww=0xFFFFFFFF) == _lib.E_INVALID_ARG
        assert call(hh=8192) == _lib.E_INVALID_ARG
        assert call(lo=None, vo=None, sh=None, va=None, co=None) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()
        assert L.infur_shapes_dev(h, P["lin"], len(l), P["vin"], len(v), P["cin"], 65, 130, P["loops"], 0, P["vertices"], 0, P["shapes"], 0, P["values"], 0,
                                  None) == _lib.E_INVALID_ARG
        assert call(ww=0, lo=None, vo=None, sh=None, va=None, co=None) == _lib.E_INVALID_ARG and "no output wanted" not in ctx.last_error()  # Simplify's order
        assert call(n=None) == _lib.E_INVALID_ARG and call(li=None) == _lib.E_INVALID_ARG and call(ve=None) == _lib.E_INVALID_ARG
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in OUTPUTS)  # no output is touched by a rejected call
        assert call(ww=8191, hh=8191) == _lib.OK  # the largest plane (the ids are read under another width: no fault, other loops)
        d.poison(*OUTPUTS)
        assert call() == _lib.OK
        ctx.synchronize()
        check_result(ref, {"loops": d.get("loops").view(np.uint32).reshape(-1, 4), "vertices": d.get("vertices").view(np.uint32),
                           "shapes": d.get("shapes").view(np.int64).reshape(-1, 12), "values": d.get("values").view(np.int64).reshape(-1, 12),
                           "counts": d.get("counts").view(np.uint32)})
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    lo, vo, co = np.full((len(l), 4), 9, np.uint32), np.full(len(v), 9, np.uint32), np.full(4, 77, np.uint32)
    sh, va = np.full((len(l), 12), 9, np.int64), np.full((ROWS, 12), 9, np.int64)
    host = lambda ww=130, li=l.ctypes.data, n=c.ctypes.data, outs=(lo, vo, sh, va, co): L.infur_shapes(  # noqa: E731
        h, li, len(l), v.ctypes.data, len(v), n, 65, ww, outs[0].ctypes.data if outs else None, len(l), outs[1].ctypes.data if outs else None, len(v),
        outs[2].ctypes.data if outs else None, len(l), outs[3].ctypes.data if outs else None, ROWS, outs[4].ctypes.data if outs else None)
    assert host(ww=0) == host(ww=8192) == host(li=None) == host(n=None) == host(outs=None) == _lib.E_INVALID_ARG
    assert (lo == 9).all() and (vo == 9).all() and (co == 77).all() and (sh == 9).all() and (va == 9).all()


def test_host_pointer_call_and_processor(ctx):
    proc, outl = Shapes(ctx), Outlines(ctx)
    assert proc.is_dirty()
    for plane in (R.smooth(65, 130), R.noise(33, 63, 21), R.stripes(7, 65)):
        hh, ww = plane.shape
        l, v, c = O.outline(plane)
        rl, rv, rs, rvals, rc = H.shapes(l, v, c, ww, rows=ROWS)
        nl, nv = len(rl), len(rv)
        oo = OutlinesOut(loops_rows=len(l), vertex_rows=len(v))
        outl.advance(plane, oo)
        out = ShapesOut(value_rows=ROWS)
        proc.advance(Shapes.input_of(oo, plane.shape), out)
        assert not proc.is_dirty() and [out.n_loops, out.n_vertices, out.status, out.largest] == rc.tolist()
        assert (out.loops == rl).all() and (out.vertices == rv).all() and (out.shapes == rs).all() and (out.values == rvals).all()
        assert [len(p[2]) for p in outlines_polygons(out.loops, out.vertices, ww)] == rl[:, 1].tolist()
        value = int(plane[0, 0])
        s = shape_summary(out.values[value])
        assert s["area"] == int((plane == value).sum()) and s["centroid"] == pytest.approx((np.nonzero(plane == value)[1].mean(),
                                                                                             np.nonzero(plane == value)[0].mean()), rel=1e-9)
        # the caller's rows beyond the counts, and beyond the rows, are left alone
        lo, vo, co = np.full((nl + 2, 4), 7, np.uint32), np.full(nv + 2, 7, np.uint32), np.zeros(4, np.uint32)
        sh, va = np.full((nl + 2, 12), 7, np.int64), np.full((ROWS + 2, 12), 7, np.int64)
        args = (ctx.h, l.ctypes.data, len(l), v.ctypes.data, len(v), c.ctypes.data, hh, ww)
        ctx.check(ctx.L.infur_shapes(*args, lo.ctypes.data, nl + 2, vo.ctypes.data, nv + 2, sh.ctypes.data, nl + 2, va.ctypes.data, ROWS, co.ctypes.data))
        assert co.tolist() == rc.tolist() and (lo[:nl] == rl).all() and (lo[nl:] == 7).all() and (vo[:nv] == rv).all() and (vo[nv:] == 7).all()
        assert (sh[:nl] == rs).all() and (sh[nl:] == 7).all() and (va[:ROWS] == rvals).all() and (va[ROWS:] == 7).all()
        for a in (lo, vo, sh):
            a[:] = 7
        ctx.check(ctx.L.infur_shapes(*args, lo.ctypes.data, 1, vo.ctypes.data, 3, sh.ctypes.data, 2, None, 0, co.ctypes.data))
        assert co.tolist() == rc.tolist() and (lo[0] == rl[0]).all() and (lo[1:] == 7).all() and (vo[:3] == rv[:3]).all() and (vo[3:] == 7).all()
        assert (sh[:2] == rs[:2]).all() and (sh[2:] == 7).all()
        for a in (lo, vo, sh, va):
            a[:] = 7
        ctx.check(ctx.L.infur_shapes(ctx.h, l.ctypes.data, len(l) - 1, v.ctypes.data, len(v), c.ctypes.data, hh, ww, lo.ctypes.data, nl, vo.ctypes.data, nv,
                                     sh.ctypes.data, nl, va.ctypes.data, 2, co.ctypes.data))  # truncated input through the host-pointer call
        assert co.tolist() == [len(l), 0, 1, 0] and (lo == 7).all() and (vo == 7).all() and (sh == 7).all()
        assert (va[:2, :10] == 0).all() and (va[:2, H.LOOP] == -1).all() and (va[2:] == 7).all()


# --------------------------------------------------------------------------- #
# 4. composition and context
# --------------------------------------------------------------------------- #
def test_calls_are_repeatable_and_contexts_agree(ctx):
    k, (l, v, c), ref = smooth_case()
    first = dev_shapes(ctx, l, v, c, 65, 130)
    again = dev_shapes(ctx, l, v, c, 65, 130)
    k2 = R.noise(135, 241, 3, seed=9)
    other = dev_shapes(ctx, *O.outline(k2), 135, 241)  # another plane, a larger one, in between
    third = dev_shapes(ctx, l, v, c, 65, 130)
    with Context(device=0) as c2:
        second_ctx = dev_shapes(c2, l, v, c, 65, 130)
    check_result(ref, first)
    for run in (again, third, second_ctx):
        assert all(run[name].tobytes() == first[name].tobytes() for name in OUTPUTS)
    assert other["counts"].tolist() != ref[4].tolist()


def test_the_call_inside_a_captured_graph(ctx):
    """capturable after one call outside the capture: the replay writes what the eager call wrote"""
    hip = _hip()
    k, (l, v, c), ref = smooth_case()
    k2 = R.smooth(65, 130, seed=7)
    l2, v2, c2 = O.outline(k2)
    assert len(l2) <= len(l) + 40 and len(v2) <= len(v) + 400
    lrows, vrows = len(l) + 40, len(v) + 400
    d = Dev(ctx, lin=lrows * 16, vin=vrows * 4, cin=12, loops=lrows * 16, vertices=vrows * 4, shapes=lrows * 96, values=ROWS * 96, counts=16)
    graph, exe = C.c_void_p(None), C.c_void_p(None)

    def put(loops, vertices, counts):
        for name, arr in (("lin", loops), ("vin", vertices)):
            buf = np.full(d.sizes[name], POISON, np.uint8)
            buf[:arr.nbytes] = arr.reshape(-1).view(np.uint8)
            d.put(name, buf)
        d.put("cin", counts)

    try:
        P, stream = d.ptr, C.c_void_p(ctx.stream)
        call = lambda: ctx.L.infur_shapes_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], 65, 130, P["loops"], lrows, P["vertices"], vrows,  # noqa: E731
                                              P["shapes"], lrows, P["values"], ROWS, P["counts"])
        put(l, v, c)
        ctx.check(call())  # the warm call allocates the scratch
        ctx.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for loops, vertices, counts, want in ((l2, v2, c2, H.shapes(l2, v2, c2, 130, rows=ROWS)), (l, v, c, ref)):
            d.poison(*OUTPUTS)
            put(loops, vertices, counts)
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            check_result(want, {"loops": d.get("loops").view(np.uint32).reshape(-1, 4), "vertices": d.get("vertices").view(np.uint32),
                                "shapes": d.get("shapes").view(np.int64).reshape(-1, 12), "values": d.get("values").view(np.int64).reshape(-1, 12),
                                "counts": d.get("counts").view(np.uint32)})
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_composition_with_regions_and_outlines_on_the_device(ctx, connectivity):
    """infur_regions_dev -> infur_outlines_dev -> infur_shapes_dev, every array where the call before left it: AREA2 / 2 is Regions'
    PIXELS and the centroid is Regions' sums, row by row"""
    k = R.smooth(65, 130)
    h, w = k.shape
    rflags, min_pixels = _lib.REGIONS_SKIP_BACKGROUND, 6
    labels, table, n_reg = R.label(k, None, connectivity, min_pixels, rflags)
    flags = SKIP | (CONN8 if connectivity == 8 else 0)
    ol, ov, oc = O.outline(labels, flags, NONE)
    rows = n_reg + 2
    ref = H.shapes(ol, ov, oc, w, rows=rows)
    lrows, vrows = len(ol) + 3, len(ov) + 3
    d = Dev(ctx, klass=h * w, labels=h * w * 4, table=rows * _lib.REGION_WORDS * 8, n=4, lin=lrows * 16, vin=vrows * 4, cin=12, loops=lrows * 16,
            vertices=vrows * 4, shapes=lrows * 96, values=rows * 96, counts=16)
    try:
        d.put("klass", k)
        P = d.ptr
        ctx.check(ctx.L.infur_regions_dev(ctx.h, P["klass"], None, h, w, connectivity, min_pixels, rflags, P["labels"], P["table"], rows, P["n"]))
        ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["labels"], 4, h, w, flags, NONE, 0, P["lin"], lrows, P["vin"], vrows, P["cin"]))
        ctx.check(ctx.L.infur_shapes_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], h, w, P["loops"], lrows, P["vertices"], vrows, P["shapes"], lrows,
                                         P["values"], rows, P["counts"]))
        ctx.synchronize()
        got = {"loops": d.get("loops").view(np.uint32).reshape(-1, 4), "vertices": d.get("vertices").view(np.uint32),
               "shapes": d.get("shapes").view(np.int64).reshape(-1, 12), "values": d.get("values").view(np.int64).reshape(-1, 12),
               "counts": d.get("counts").view(np.uint32)}
        check_result(ref, got)
        tab = d.get("table").view(np.uint64).reshape(rows, _lib.REGION_WORDS)
        assert d.get("n").view(np.uint32)[0] == n_reg
        for i in range(n_reg):
            ys, xs = np.nonzero(labels == i)
            pixels = len(xs)
            assert int(tab[i, _lib.STAT_PIXELS]) == pixels and got["values"][i, H.AREA2] == 2 * pixels
            # 6 * integral of x over the pixel squares = 3 * sum(2x + 1): Regions' sum of x, exactly
            assert int(tab[i, _lib.STAT_SUM_X]) == int(xs.sum()) and int(tab[i, _lib.STAT_SUM_Y]) == int(ys.sum())
            assert got["values"][i, H.M10_6] == 3 * (2 * int(tab[i, _lib.STAT_SUM_X]) + pixels)
            assert got["values"][i, H.M01_6] == 3 * (2 * int(tab[i, _lib.STAT_SUM_Y]) + pixels)
            assert got["values"][i, H.OUTER] >= 1 and got["shapes"][got["values"][i, H.LOOP], H.AREA2] > 0
            assert got["loops"][got["values"][i, H.LOOP], 2] == i
    finally:
        d.free()


# --------------------------------------------------------------------------- #
# 5. the fused frame path
# --------------------------------------------------------------------------- #
def frame_reference(labels, connectivity, rows):
    flags = SKIP | (CONN8 if connectivity == 8 else 0)
    o = O.outline(labels, flags, NONE)
    return o, H.shapes(*o, labels.shape[1], rows=rows)


@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_regions_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    for (h, w), connectivity, min_pixels in (((48, 64), 8, 0), ((61, 97), 4, 5)):
        frame = W.synth_frame(h, w, index=h)
        rflags = _lib.REGIONS_SKIP_BACKGROUND if min_pixels else 0
        want = fp.advance_regions(frame, 1.0, decode, connectivity, min_pixels, rflags, table_rows=h * w)
        rows = want.n + 3
        o, (rl, rv, rs, rvals, rc) = frame_reference(want.labels, connectivity, rows)
        r = fp.advance_shapes(frame, 1.0, decode, connectivity, min_pixels, rflags, table_rows=rows, want_labels=True, want_klass=True, want_conf=True,
                              want_scaled=True)
        assert r.counts == tuple(rc.tolist()) and r.n_regions == want.n and r.shape == (h, w) and r.scaled.shape == (h, w, 3)
        assert (r.loops == rl).all() and (r.vertices == rv).all() and (r.shapes == rs).all() and (r.values == rvals).all()
        assert (r.labels == want.labels).all() and (r.klass == want.klass).all() and (r.conf == want.conf).all() and (r.table == want.table[:rows]).all()
        for i in range(want.n):  # row i is region i
            assert r.values[i, H.AREA2] == 2 * int(want.table[i, _lib.STAT_PIXELS])
        # short tables, no dense plane; an edge capacity that is just enough, and one that is not
        q = fp.advance_shapes(frame, 1.0, decode, connectivity, min_pixels, rflags, table_rows=2, max_edges=int(o[2][2]), loops_rows=2, vertex_rows=3,
                              shape_rows=1)
        assert q.counts == tuple(rc.tolist()) and (q.loops == rl[:2]).all() and (q.vertices == rv[:3]).all() and (q.shapes == rs[:1]).all()
        assert (q.values == H.shapes(*o, w, rows=2)[3]).all() and q.labels is None and q.klass is None and q.n_regions == want.n
        q = fp.advance_shapes(frame, 1.0, decode, connectivity, min_pixels, rflags, table_rows=2, max_edges=int(o[2][2]) - 1)
        assert q.counts == (0, 0, 0, 0) and len(q.loops) == 0 and len(q.vertices) == 0 and len(q.shapes) == 0
        assert (q.values[:, :10] == 0).all() and (q.values[:, H.LOOP] == -1).all()


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    for hh, ww in ((48, 64), (61, 97)):
        frame = W.synth_frame(hh, ww, index=2)
        want = FramePath(ctx).advance_regions(frame, 1.0, SOFTMAX, 8, 0, 0, table_rows=hh * ww)
        rows = want.n + 2
        _, ref = frame_reference(want.labels, 8, rows)
        nl, nv = len(ref[0]), len(ref[1])
        d = Dev(ctx, bgr=frame.nbytes, labels=hh * ww * 4, table=rows * _lib.REGION_WORDS * 8, n=4, loops=(nl + 2) * 16, vertices=(nv + 2) * 4,
                shapes=(nl + 2) * 96, values=rows * 96, counts=16)
        try:
            d.put("bgr", frame)
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            P = d.ptr
            for dense in (True, False):
                d.poison("labels", "table", "n", *OUTPUTS)
                ctx.check(L.infur_frame_shapes_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 8, 0, 0, None, None, 0, P["labels"] if dense else None, hh * ww * 4,
                                                   P["table"] if dense else None, rows, P["n"] if dense else None, None, C.byref(ow), C.byref(oh), 0,
                                                   P["loops"], nl + 2, P["vertices"], nv + 2, P["shapes"], nl + 2, P["values"], P["counts"]))
                ctx.synchronize()
                assert (ow.value, oh.value) == (ww, hh)
                check_result(ref, {"loops": d.get("loops").view(np.uint32).reshape(-1, 4), "vertices": d.get("vertices").view(np.uint32),
                                   "shapes": d.get("shapes").view(np.int64).reshape(-1, 12), "values": d.get("values").view(np.int64).reshape(-1, 12),
                                   "counts": d.get("counts").view(np.uint32)})
                if dense:
                    assert (d.get("labels").view(np.uint32).reshape(hh, ww) == want.labels).all() and d.get("n").view(np.uint32)[0] == want.n
                    assert (d.get("table").view(np.uint64).reshape(rows, -1)[:want.n] == want.table).all()
                else:
                    assert all((d.get(name) == POISON).all() for name in ("labels", "table", "n"))
        finally:
            d.free()


def test_fused_rules_and_error_codes(ctx, model):
    """the capacity errors and the check order are infur_frame_regions' own"""
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    npix = 48 * 64
    labels, n = np.full((48, 64), 9, np.uint32), np.full(1, 9, np.uint32)
    values, counts = np.full((16, 12), 9, np.int64), np.full(4, 9, np.uint32)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731

    def call(lib=L, handle=h, decode=0, mode=0, factor=1.0, conn=8, flags=0, plane_cap=npix, kl=None, lb=labels, lcap=npix * 4, nr=n, va=values, cn=counts,
             scaled=None):
        return lib.infur_frame_shapes(handle, p(frame), 64, 48, factor, mode, decode, conn, 0, flags, p(kl), None, plane_cap, p(lb), lcap, None, 16, p(nr),
                                      p(scaled), C.byref(ow), C.byref(oh), 0, None, 0, None, 0, None, 0, p(va), p(cn))

    want = FramePath(ctx).advance_regions(frame, 1.0, RAW, 8, 0, 0, table_rows=npix)
    _, ref = frame_reference(want.labels, 8, 16)
    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48)
    assert (values == ref[3]).all() and (counts == ref[4]).all() and (labels == want.labels).all() and n[0] == want.n
    assert call(conn=5) == _lib.E_INVALID_ARG and "connectivity" in ctx.last_error()
    assert call(flags=2) == _lib.E_INVALID_ARG and "regions flags" in ctx.last_error()
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) != _lib.OK and call(factor=-1.0) == _lib.E_INVALID_SCALE
    assert call(lcap=npix * 4 - 1) == _lib.E_CAPACITY and "label plane" in ctx.last_error()
    klass = np.full((48, 64), 9, np.uint8)
    assert call(kl=klass, plane_cap=npix - 1) == _lib.E_CAPACITY and "a plane needs" in ctx.last_error() and (klass == 9).all()
    assert call(lb=None, nr=None, va=None, cn=None) == _lib.E_INVALID_ARG
    assert call(kl=klass) == _lib.OK and (klass == want.klass).all()
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_shapes(frame, 0.5, RAW, want_scaled=True)
        assert r.loops is None and r.values is None and r.counts is None and r.n_regions is None and r.scaled.shape == (24, 32, 3)
        for x in (labels, n, values, counts):
            x[:] = 9
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED
        assert (scaled == FramePath(c).advance_segments(frame, 1.0, RAW, want_scaled=True).scaled).all()
        assert all((x == 9).all() for x in (labels, n, values, counts))
        # a label plane that is too short: whatever infur_frame_regions answers without a model, in its own words
        want_rc = c.L.infur_frame_regions(c.h, p(frame), 64, 48, 1.0, 0, 0, 8, 0, 0, None, None, npix, p(labels), 3, None, 0, p(n), None, C.byref(ow),
                                          C.byref(oh))
        want_msg = c.last_error()
        assert call(lib=c.L, handle=c.h, lcap=3) == want_rc != _lib.OK and c.last_error() == want_msg
        assert all((x == 9).all() for x in (labels, n, values, counts))


def test_shapes_calls_leave_the_existing_legs_and_the_cached_graphs_alone(blob50):
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
        before = [fg.advance_regions(fr, 1.0, SOFTMAX) for fr in frames]  # the existing leg, before any Shapes call on this context
        for it in range(8):
            fr = frames[it % 4]
            kw = dict(factor=1.0, decode=SOFTMAX if it & 1 else RAW, connectivity=4 if it & 4 else 8, min_pixels=8 if it & 2 else 0, table_rows=2048,
                      want_labels=bool(it & 1))
            s, e = fg.advance_shapes(fr, **kw), fe.advance_shapes(fr, **kw)  # (mem_gen unchanged: no capture, no graph dropped, below)
            assert s.n_regions == e.n_regions and s.counts == e.counts
            assert all(getattr(s, f).tobytes() == getattr(e, f).tobytes() for f in ("loops", "vertices", "shapes", "values", "table"))
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a shapes call caused a capture"
        assert cached1 >= cached0, "a shapes call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the shapes calls were not replayed"
        for fr, b4 in zip(frames, before):  # and after: the same bytes
            now = fg.advance_regions(fr, 1.0, SOFTMAX)
            assert now.n == b4.n and all(getattr(now, f).tobytes() == getattr(b4, f).tobytes() for f in ("klass", "conf", "labels", "table"))


# --------------------------------------------------------------------------- #
# 6. the command line
# --------------------------------------------------------------------------- #
def test_cli_describes_every_region(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    (tmp_path / "clip.bgr24").write_bytes(b"".join(f.tobytes() for f in frames))
    cmd = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input",
           str(tmp_path / "clip.bgr24"), "--regions", "--shapes", "--connectivity", "4", "--min-pixels", "3", "--skip-background", "--max-regions",
           str(96 * 128), "--regions-out", str(tmp_path / "labels.u32"), "--hulls-out", str(tmp_path / "hulls.bin")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    blob = np.frombuffer((tmp_path / "hulls.bin").read_bytes(), np.uint32)
    at = 0
    assert len(lines) == 2
    for i in range(2):
        n = len(lines[i]["regions"])
        assert n == lines[i]["n_regions"] > 0
        _, (rl, rv, rs, rvals, rc) = frame_reference(labels[i], 4, n)
        assert blob[at:at + 4].tolist() == rc.tolist() and lines[i]["n_hull_vertices"] == rc[1]
        at += 4
        assert (blob[at:at + rl.size].reshape(-1, 4) == rl).all()
        at += rl.size
        assert (blob[at:at + len(rv)] == rv).all()
        at += len(rv)
        for region, row in zip(lines[i]["regions"], rvals):
            loop = int(row[H.LOOP])
            want = shape_summary(row, rs[loop], np.array(H.hull_xy(rl, rv, loop, 128)).T)
            assert region["shape"] == json.loads(json.dumps(want)) and region["shape"]["area"] == region["pixels"]
    assert at == len(blob)
    bad = subprocess.run(cmd[:-2] + ["--anchors"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert bad.returncode != 0 and "--shapes does not combine with --anchors" in bad.stderr
