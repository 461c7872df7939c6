"""Simplify on the GPU: loop records, vertices and counts of ``infur_simplify*`` and of the fused ``infur_frame_polygons*`` against
tests/simplify_ref.py.  The kept set is a function of the loop alone, so every comparison is ``==`` on whole arrays.  Every
output buffer is filled with a poison byte first: what a call must leave alone still holds it afterwards, and what it must write
owes nothing to an initialisation."""
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
from infur_amd.processors import (Context, FramePath, Model, ModelCmd, Outlines, OutlinesOut, Simplify, SimplifyCmd, SimplifyOut,
                                  outlines_by_value, outlines_polygons)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import simplify_ref as S  # noqa: E402
import test_gpu_outlines as TO  # noqa: E402  (its poisoned, guard-padded device buffers, its families and its shapes)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
SKIP, CONN8 = _lib.OUTLINES_SKIP, _lib.OUTLINES_CONN8
NONE = 0xFFFFFFFF
POISON, POISON32 = TO.POISON, TO.POISON32
Dev = TO.Dev
TOLS = (0, 8, 11, 12, 16, 32, 4096, 65535)


@functools.lru_cache(maxsize=None)
def family_outlines(conn):
    """[(name, plane, (loops, vertices, counts))] of the nine families at the eight shapes: computed once, shared, never changed"""
    out = []
    for h, w in TO.SHAPES:
        for name, k in TO.families(h, w):
            out.append((f"{name} {h}x{w}", k, O.outline(k, conn)))
    return out


@functools.lru_cache(maxsize=None)
def family_reference(conn, tol16):
    return [S.simplify(l, v, c, k.shape[1], tol16) for _, k, (l, v, c) in family_outlines(conn)]


def dev_simplify(ctx, loops, vertices, counts, h, w, tol16, loops_rows_in=None, vertex_rows_in=None, loops_rows_out=None, vertex_rows_out=None,
                 want=("loops", "vertices", "counts"), spare=5):
    """infur_simplify_dev on poisoned device buffers -> (loops_out [loops_rows_out, 4], vertices_out [vertex_rows_out], counts_out
    [4]) as the buffers hold them, None for what was not wanted (and that buffer is checked to be untouched).  The input buffers
    hold loops_rows_in records and vertex_rows_in vertices: what the arrays do not fill stays poisoned."""
    loops, vertices = np.asarray(loops, np.uint32).reshape(-1, 4), np.asarray(vertices, np.uint32)
    lin = len(loops) + spare if loops_rows_in is None else loops_rows_in
    vin = len(vertices) + spare if vertex_rows_in is None else vertex_rows_in
    lout = len(loops) + spare if loops_rows_out is None else loops_rows_out
    vout = len(vertices) + spare if vertex_rows_out is None else vertex_rows_out
    d = Dev(ctx, lin=lin * 16, vin=vin * 4, cin=12, loops=lout * 16, vertices=vout * 4, counts=16)
    try:
        for name, arr, rows in (("lin", loops, lin), ("vin", vertices, vin)):
            buf = np.full(d.sizes[name], POISON, np.uint8)
            part = arr[:rows].reshape(-1).view(np.uint8)
            buf[:len(part)] = part
            d.put(name, buf)
        d.put("cin", np.asarray(counts, np.uint32)[:3] if len(counts) >= 3 else np.array(list(counts) + [0], np.uint32))
        before = {name: d.get(name).tobytes() for name in ("lin", "vin", "cin")}
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_simplify_dev(ctx.h, d.ptr["lin"], lin, d.ptr["vin"], vin, d.ptr["cin"], h, w, tol16, p("loops"), lout, p("vertices"), vout,
                                           p("counts")))
        ctx.synchronize()
        got = (d.get("loops").view(np.uint32).reshape(lout, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
        assert all(d.get(name).tobytes() == b for name, b in before.items())  # the input is an input
        for name, g in zip(("loops", "vertices", "counts"), got):
            if name not in want:
                assert (g.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return tuple(g if name in want else None for name, g in zip(("loops", "vertices", "counts"), got))
    finally:
        d.free()


def check_result(ref, got, name=""):
    """whole arrays against the reference's; what lies behind the counts still holds the poison"""
    (rl, rv, rc), (loops, vertices, counts) = ref, got
    assert counts.tolist() == rc.tolist(), (name, counts, rc)
    assert (loops[:len(rl)] == rl).all() and (loops[len(rl):] == POISON32).all(), name
    assert (vertices[:len(rv)] == rv).all() and (vertices[len(rv):] == POISON32).all(), name


# --------------------------------------------------------------------------- #
# 1. infur_simplify_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conn", [0, CONN8])
def test_families_equal_the_reference(ctx, conn):
    assert ctx.L.infur_features() & _lib.FEATURE_SIMPLIFY  # (the first line: fails on a library without the feature)
    total = {}
    for tol16 in TOLS:
        for (name, k, (l, v, c)), ref in zip(family_outlines(conn), family_reference(conn, tol16)):
            h, w = k.shape
            check_result(ref, dev_simplify(ctx, l, v, c, h, w, tol16), (name, tol16))
            total[tol16] = total.get(tol16, 0) + int(ref[2][1])
        print(f"conn {conn} tol16 {tol16}: {total[tol16]} vertices kept")
    assert total[0] > total[11] > total[16] > total[32] >= total[4096] >= total[65535] > 0
    # what the families are for: a rectangle keeps its four corners whatever the tolerance (two anchors on a diagonal, the other
    # two corners h*w / sqrt(h^2 + w^2) off it) until the tolerance exceeds that distance
    at = [n for n, _, _ in family_outlines(conn)].index("single 65x130")
    assert [family_reference(conn, t)[at][2].tolist() for t in (0, 16, 32)] == [[1, 4, 0, 0]] * 3
    assert family_reference(conn, 65535)[at][2].tolist() == [1, 2, 1, 0]


@pytest.mark.parametrize("conn", [0, CONN8])
def test_families_from_outlines_left_on_the_device(ctx, conn):
    """infur_outlines_dev, then infur_simplify_dev on what it left in device memory, rows and all"""
    for i, (name, k, (l, v, c)) in enumerate(family_outlines(conn)):
        h, w = k.shape
        lrows, vrows = len(l) + 3, len(v) + 3
        d = Dev(ctx, plane=k.nbytes, lin=lrows * 16, vin=vrows * 4, cin=12, loops=lrows * 16, vertices=vrows * 4, counts=16)
        try:
            d.put("plane", k)
            P = d.ptr
            ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["plane"], 1, h, w, conn, 0, 0, P["lin"], lrows, P["vin"], vrows, P["cin"]))
            for tol16 in TOLS:
                d.poison("loops", "vertices", "counts")
                ctx.check(ctx.L.infur_simplify_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], h, w, tol16, P["loops"], lrows, P["vertices"], vrows,
                                                   P["counts"]))
                ctx.synchronize()
                got = (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
                check_result(family_reference(conn, tol16)[i], got, (name, tol16))
            assert d.get("cin").view(np.uint32).tolist() == c.tolist() and (d.get("lin").view(np.uint32).reshape(-1, 4)[:len(l)] == l).all()
        finally:
            d.free()


@pytest.mark.parametrize("n_vertices", [62, 64, 66, 126, 128, 130])
def test_wave_edges_on_the_stairs(ctx, n_vertices):
    """one loop of n_vertices around a right triangle of k unit steps: its 45-degree corners tie exactly in D, so the smallest-index
    rule decides, and the loop ends just below, at and just above one and two strides of the wave"""
    k = (n_vertices - 2) // 2
    plane = S.stairs(k)
    l, v, c = O.outline(plane, SKIP, 0)
    assert c.tolist()[:2] == [1, n_vertices]
    for tol16 in TOLS:
        ref = S.simplify(l, v, c, k, tol16)
        check_result(ref, dev_simplify(ctx, l, v, c, k, k, tol16), (n_vertices, tol16))
        S.check_invariants(l, v, c, k, tol16, *ref)
    # below 0.707 px the outer corners stay, at 12/16 the staircase is its chord
    assert S.simplify(l, v, c, k, 11)[2][1] > 3 == S.simplify(l, v, c, k, 12)[2][1]


@functools.lru_cache(maxsize=None)
def comb_outline():
    plane = S.comb(130, 2100)
    return plane.shape, O.outline(plane, SKIP, 0)


def test_comb_plane_one_long_loop_and_more_than_1024_block_sums(ctx):
    """one loop of more than 2^16 vertices; with 1.1 M vertex rows declared the scan of the block sums takes a second pass"""
    (h, w), (l, v, c) = comb_outline()
    assert c[0] == 1 and c[1] > 1 << 16
    rows = 1100 * 1024
    for tol16 in (16, 32):
        ref = S.simplify(l, v, c, w, tol16)
        assert 2 < ref[2][1] < c[1]
        check_result(ref, dev_simplify(ctx, l, v, c, h, w, tol16, vertex_rows_in=rows), tol16)
        print(f"comb {h}x{w}: {int(c[1])} vertices -> {int(ref[2][1])} at tol16 {tol16}")


def test_self_touching_loops(ctx):
    """the checkerboard under 8-connectivity: chains that pass a saddle vertex twice, so that segments with L == 0 occur"""
    k = R.checkerboard(7, 9)
    l, v, c = O.outline(k, CONN8)
    seen = []
    real = S.keep_loop

    def spy(x, y, tol16):
        n = len(x)
        seen.append(any(x[a] == x[b % n] and y[a] == y[b % n] for a in range(n) for b in range(a + 2, n + 1) if (a, b) != (0, n)))
        return real(x, y, tol16)

    S.simplify(l, v, c, 9, 16, keep_fn=spy)
    assert any(seen)  # a loop that touches itself is there
    for tol16 in TOLS:
        for plane in (k, R.checkerboard(33, 63)):
            l, v, c = O.outline(plane, CONN8)
            ref = S.simplify(l, v, c, plane.shape[1], tol16)
            check_result(ref, dev_simplify(ctx, l, v, c, *plane.shape, tol16), tol16)
            S.check_invariants(l, v, c, plane.shape[1], tol16, *ref)
    # a segment whose ends coincide (L == 0) needs a loop whose vertices are all one point: no plane has one, the rule covers it
    ids = np.full(70 + 3, 2 * 10 + 3, np.uint32)
    hand = np.array([[0, 70, 1, 0], [70, 3, 2, 4]], np.uint32)
    ref = S.simplify(hand, ids, [2, 73], 9, 0)
    assert ref[0].tolist() == [[0, 2, 1, 0], [2, 2, 2, 4]] and ref[2].tolist() == [2, 4, 2, 0]
    check_result(ref, dev_simplify(ctx, hand, ids, np.array([2, 73, 0], np.uint32), 7, 9, 0))


# --------------------------------------------------------------------------- #
# 2. calling modes
# --------------------------------------------------------------------------- #
def smooth_case(tol16=12):
    k = R.smooth(65, 130)
    l, v, c = O.outline(k)
    return k, (l, v, c), S.simplify(l, v, c, 130, tol16)


def test_each_output_alone_equals_all_together(ctx):
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    for want in (("loops",), ("vertices",), ("counts",), ("loops", "counts"), ("vertices", "counts"), ("loops", "vertices")):
        loops, vertices, counts = dev_simplify(ctx, l, v, c, 65, 130, 12, want=want, spare=0)
        assert loops is None or (loops[:len(rl)] == rl).all(), want
        assert vertices is None or ((vertices[:len(rv)] == rv).all() and (vertices[len(rv):] == POISON32).all()), want
        assert counts is None or counts.tolist() == rc.tolist(), want
    # pointers with no rows are no tables
    loops, vertices, counts = dev_simplify(ctx, l, v, c, 65, 130, 12, loops_rows_out=0, vertex_rows_out=0)
    assert counts.tolist() == rc.tolist()


def test_truncated_outputs_keep_the_full_prefix_sum(ctx):
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    nl, nv = len(rl), len(rv)
    assert nl > 8 and nv > 8 and rc[2] > 0
    for lrows, vrows in ((0, nv), (1, nv), (nl - 1, nv), (nl, nv), (nl + 7, nv), (nl, 0), (nl, 1), (nl, nv - 1), (nl, nv + 7), (1, 1)):
        loops, vertices, counts = dev_simplify(ctx, l, v, c, 65, 130, 12, loops_rows_out=lrows, vertex_rows_out=vrows)
        assert counts.tolist() == rc.tolist(), (lrows, vrows)  # the full counts: that is how a caller sees truncation
        ml, mv = min(nl, lrows), min(nv, vrows)
        assert (loops[:ml] == rl[:ml]).all() and (loops[ml:] == POISON32).all(), (lrows, vrows)  # OFFSET' is the full prefix sum
        assert (vertices[:mv] == rv[:mv]).all() and (vertices[mv:] == POISON32).all(), (lrows, vrows)


def test_calls_are_repeatable_and_contexts_agree(ctx):
    k, (l, v, c), ref = smooth_case(16)
    first = dev_simplify(ctx, l, v, c, 65, 130, 16)
    again = dev_simplify(ctx, l, v, c, 65, 130, 16)
    k2 = R.noise(135, 241, 3, seed=9)
    other = dev_simplify(ctx, *O.outline(k2), 135, 241, 16)  # another plane, a larger one, in between
    third = dev_simplify(ctx, l, v, c, 65, 130, 16)
    with Context(device=0) as c2:
        second_ctx = dev_simplify(c2, l, v, c, 65, 130, 16)
    check_result(ref, first)
    for run in (again, third, second_ctx):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run, first))
    assert other[2].tolist() != ref[2].tolist()


def test_status_bit_0_truncated_input(ctx):
    """input counts above the declared rows: {n_loops, 0, 0, 1} and nothing else"""
    k, (l, v, c), _ = smooth_case()
    nl, nv = len(l), len(v)
    for lin, vin in ((nl - 1, nv), (nl, nv - 1), (1, 1), (0, nv), (nl, 0), (0, 0)):
        loops, vertices, counts = dev_simplify(ctx, l, v, c, 65, 130, 12, loops_rows_in=lin, vertex_rows_in=vin, loops_rows_out=nl, vertex_rows_out=nv)
        assert counts.tolist() == [nl, 0, 0, _lib.SIMPLIFY_TRUNCATED], (lin, vin)
        assert (loops == POISON32).all() and (vertices == POISON32).all(), (lin, vin)
        assert S.simplify(l, v, c, 130, 12, lin, vin)[2].tolist() == counts.tolist()
        assert S.emulate(l, v, c, 130, 12, lin, vin, nl, nv)[2].tolist() == counts.tolist()
    # rows exactly as large as the counts are not truncated
    assert dev_simplify(ctx, l, v, c, 65, 130, 12, loops_rows_in=nl, vertex_rows_in=nv)[2][3] == 0


def test_status_bit_1_malformed_records(ctx):
    """COUNT < 2 or OFFSET + COUNT > n_vertices: COUNT' = 0, the other loops as ever.  No record here points outside the vertices the
    test itself allocated: the buffers hold `spare` poisoned rows behind the arrays, and the bad ranges end inside them"""
    k, (l, v, c), _ = smooth_case()
    nl, nv = len(l), len(v)
    spare = 64
    for tol16 in (0, 12, 32):
        bad = l.copy()
        bad[2, S.COUNT] = 1                                  # too short; its vertices become a gap
        bad[5, S.COUNT] = 0
        bad[nl - 1, S.COUNT] += 3                            # ends 3 beyond n_vertices (inside the spare rows)
        bad[nl - 3, S.OFFSET], bad[nl - 3, S.COUNT] = nv + 9, 4  # begins beyond n_vertices (inside the spare rows)
        ref = S.simplify(bad, v, c, 130, tol16)
        assert ref[2][3] == _lib.SIMPLIFY_MALFORMED and (ref[0][[2, 5, nl - 1, nl - 3], S.COUNT] == 0).all()
        assert ref[0][nl - 3, S.OFFSET] == ref[2][1]  # OFFSET' of a record that begins beyond the vertices: all kept vertices lie before it
        got = dev_simplify(ctx, bad, v, c, 65, 130, tol16, spare=spare)
        check_result(ref, got, tol16)
        assert all((a == b).all() for a, b in zip(S.emulate(bad, v, c, 130, tol16), ref))
        good = S.simplify(l, v, c, 130, tol16)[0]
        keep = np.ones(nl, bool)
        keep[[2, 5, nl - 1, nl - 3]] = False
        assert (ref[0][keep][:, S.COUNT] == good[keep][:, S.COUNT]).all()  # the well-formed loops are simplified as ever


def test_idempotence_on_the_device(ctx):
    for plane, flags in ((R.smooth(65, 130), 0), (R.noise(33, 63, 3), CONN8), (S.stairs(31), SKIP)):
        h, w = plane.shape
        l, v, c = O.outline(plane, flags, 0)
        for tol16 in (0, 11, 16, 32):
            l1, v1, c1 = dev_simplify(ctx, l, v, c, h, w, tol16, spare=0)
            n1 = int(c1[1])
            l2, v2, c2 = dev_simplify(ctx, l1, v1[:n1], c1, h, w, tol16, loops_rows_out=len(l1), vertex_rows_out=len(v1))
            assert c2.tolist() == c1.tolist() and l2.tobytes() == l1.tobytes() and (v2[:n1] == v1[:n1]).all() and (v2[n1:] == POISON32).all()


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    d = Dev(ctx, lin=l.nbytes, vin=v.nbytes, cin=12, loops=l.nbytes, vertices=v.nbytes, counts=16)
    try:
        d.put("lin", l)
        d.put("vin", v)
        d.put("cin", c)
        P = d.ptr
        call = lambda hh=65, ww=130, tol=12, li=P["lin"], ve=P["vin"], n=P["cin"], lo=P["loops"], vo=P["vertices"], co=P["counts"]: L.infur_simplify_dev(  # noqa: E731
            h, li, len(l), ve, len(v), n, hh, ww, tol, lo, len(l), vo, len(v), co)
        assert call(ww=0) == _lib.E_INVALID_ARG and call(ww=8192) == _lib.E_INVALID_ARG and call(ww=0xFFFFFFFF) == _lib.E_INVALID_ARG
        assert call(hh=8192) == _lib.E_INVALID_ARG
        assert call(tol=65536) == _lib.E_INVALID_ARG and "tol16" in ctx.last_error()
        assert call(lo=None, vo=None, co=None) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()
        assert L.infur_simplify_dev(h, P["lin"], len(l), P["vin"], len(v), P["cin"], 65, 130, 12, P["loops"], 0, P["vertices"], 0, None) == _lib.E_INVALID_ARG
        assert call(n=None) == _lib.E_INVALID_ARG and call(li=None) == _lib.E_INVALID_ARG and call(ve=None) == _lib.E_INVALID_ARG
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("loops", "vertices", "counts"))  # no output is touched by a rejected call
        assert call(ww=8191, hh=8191, tol=65535) == _lib.OK  # the largest plane and tolerance (the ids are read under another width: no fault, other loops)
        d.poison("loops", "vertices", "counts")
        assert call() == _lib.OK
        ctx.synchronize()
        check_result((rl, rv, rc), (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32)))
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    lo, vo, co = np.full((len(l), 4), 9, np.uint32), np.full(len(v), 9, np.uint32), np.full(4, 77, np.uint32)
    host = lambda ww=130, tol=12, li=l.ctypes.data, n=c.ctypes.data, lout=lo.ctypes.data, vout=vo.ctypes.data, cout=co.ctypes.data: L.infur_simplify(  # noqa: E731
        h, li, len(l), v.ctypes.data, len(v), n, 65, ww, tol, lout, len(l), vout, len(v), cout)
    assert host(ww=0) == host(ww=8192) == host(tol=65536) == host(li=None) == host(n=None) == host(lout=None, vout=None, cout=None) == _lib.E_INVALID_ARG
    assert (lo == 9).all() and (vo == 9).all() and (co == 77).all()
    with pytest.raises(Exception):
        Simplify(ctx).control(SimplifyCmd.Tol16(65536))
    with pytest.raises(Exception):
        SimplifyCmd.Tolerance(-1.0)
    assert SimplifyCmd.Tolerance(0.75).tol16 == 12 and SimplifyCmd.Tolerance(1.0).tol16 == 16 and SimplifyCmd.Tolerance(0.7).tol16 == 11


def test_host_pointer_call_and_processor(ctx):
    proc = Simplify(ctx)
    assert proc.is_dirty() and proc.tol16 == 16
    outl = Outlines(ctx)
    for plane in (R.smooth(65, 130), R.noise(33, 63, 21), R.stripes(7, 65)):
        hh, ww = plane.shape
        l, v, c = O.outline(plane)
        oo = OutlinesOut(loops_rows=len(l), vertex_rows=len(v))
        outl.advance(plane, oo)
        for tol16 in (11, 16):
            rl, rv, rc = S.simplify(l, v, c, ww, tol16)
            nl, nv = len(rl), len(rv)
            out = SimplifyOut()
            proc.control(SimplifyCmd.Tol16(tol16)).advance(Simplify.input_of(oo, plane.shape), out)
            assert not proc.is_dirty() and [out.n_loops, out.n_vertices, out.n_degenerate, out.status] == rc.tolist()
            assert out.loops.shape == (nl, 4) and (out.loops == rl).all() and (out.vertices == rv).all()
            # the helpers of Outlines work unchanged on the simplified arrays
            polys = outlines_polygons(out.loops, out.vertices, ww)
            assert len(polys) == nl and [len(p[2]) for p in polys] == rl[:, S.COUNT].tolist()
            assert [(p[0], p[1]) for p in polys] == [(p[0], p[1]) for p in outlines_polygons(l, v, ww)]
            assert sorted(outlines_by_value(out.loops, out.vertices, ww)) == np.unique(plane).tolist()
            # the caller's records and vertices beyond the counts, and beyond the rows, are left alone
            lo, vo, co = np.full((nl + 2, 4), 7, np.uint32), np.full(nv + 2, 7, np.uint32), np.zeros(4, np.uint32)
            ctx.check(ctx.L.infur_simplify(ctx.h, l.ctypes.data, len(l), v.ctypes.data, len(v), c.ctypes.data, hh, ww, tol16, lo.ctypes.data, nl + 2,
                                           vo.ctypes.data, nv + 2, co.ctypes.data))
            assert co.tolist() == rc.tolist() and (lo[:nl] == rl).all() and (lo[nl:] == 7).all() and (vo[:nv] == rv).all() and (vo[nv:] == 7).all()
            lo[:], vo[:] = 7, 7
            ctx.check(ctx.L.infur_simplify(ctx.h, l.ctypes.data, len(l), v.ctypes.data, len(v), c.ctypes.data, hh, ww, tol16, lo.ctypes.data, 1,
                                           vo.ctypes.data, 3, co.ctypes.data))
            assert co.tolist() == rc.tolist() and (lo[0] == rl[0]).all() and (lo[1:] == 7).all() and (vo[:3] == rv[:3]).all() and (vo[3:] == 7).all()
            # truncated input through the host-pointer call
            lo[:], vo[:] = 7, 7
            ctx.check(ctx.L.infur_simplify(ctx.h, l.ctypes.data, len(l) - 1, v.ctypes.data, len(v), c.ctypes.data, hh, ww, tol16, lo.ctypes.data, nl,
                                           vo.ctypes.data, nv, co.ctypes.data))
            assert co.tolist() == [len(l), 0, 0, 1] and (lo == 7).all() and (vo == 7).all()
        assert proc.control(SimplifyCmd.Tol16(16)).is_dirty() is False and proc.control(SimplifyCmd.Tol16(32)).is_dirty()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_composition_with_regions_and_outlines_on_the_device(ctx, connectivity):
    """infur_regions_dev -> infur_outlines_dev -> infur_simplify_dev, every array where the call before left it"""
    k = R.smooth(65, 130)
    h, w = k.shape
    rflags, min_pixels, tol16 = _lib.REGIONS_SKIP_BACKGROUND, 6, 12
    labels, table, n_reg = R.label(k, None, connectivity, min_pixels, rflags)
    flags = SKIP | (CONN8 if connectivity == 8 else 0)
    ol, ov, oc = O.outline(labels, flags, NONE)
    ref = S.simplify(ol, ov, oc, w, tol16)
    lrows, vrows = len(ol) + 3, len(ov) + 3
    d = Dev(ctx, klass=h * w, labels=h * w * 4, lin=lrows * 16, vin=vrows * 4, cin=12, loops=lrows * 16, vertices=vrows * 4, counts=16)
    try:
        d.put("klass", k)
        P = d.ptr
        ctx.check(ctx.L.infur_regions_dev(ctx.h, P["klass"], None, h, w, connectivity, min_pixels, rflags, P["labels"], None, 0, None))
        ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["labels"], 4, h, w, flags, NONE, 0, P["lin"], lrows, P["vin"], vrows, P["cin"]))
        ctx.check(ctx.L.infur_simplify_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], h, w, tol16, P["loops"], lrows, P["vertices"], vrows, P["counts"]))
        ctx.synchronize()
        got = (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
        check_result(ref, got)
        by = outlines_by_value(got[0][:len(ol)], got[1], w)  # one object's polygon with its holes, simplified
        assert sorted(by) == list(range(n_reg))
    finally:
        d.free()


# --------------------------------------------------------------------------- #
# 3. the fused frame path
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_segments_then_the_references(ctx, model, decode):
    fp = FramePath(ctx)
    for h, w in ((48, 64), (61, 97)):
        frame = W.synth_frame(h, w, index=h)
        s = fp.advance_segments(frame, 1.0, decode)
        ol, ov, oc = O.outline(s.klass)
        for tol16 in (11, 16):
            rl, rv, rc = S.simplify(ol, ov, oc, w, tol16)
            r = fp.advance_polygons(frame, 1.0, decode, tol16, loops_rows=len(rl) + 1, vertex_rows=len(rv) + 1, want_scaled=True)
            assert list(r.counts) == rc.tolist() and (r.loops == rl).all() and (r.vertices == rv).all() and r.shape == (h, w), (h, w, tol16)
            assert r.stats.tobytes() == s.stats.tobytes() and r.scaled.shape == (h, w, 3)
        # skip, 8-connectivity, an edge capacity that is just enough, truncated tables; no statistics
        skip_value = int(s.klass[0, 0])
        sl, sv, sc = O.outline(s.klass, SKIP | CONN8, skip_value)
        ql, qv, qc = S.simplify(sl, sv, sc, w, 16)
        q = fp.advance_polygons(frame, 1.0, decode, 16, skip=skip_value, connectivity=8, max_edges=int(sc[2]), loops_rows=2, vertex_rows=3, want_stats=False)
        assert list(q.counts) == qc.tolist() and q.stats is None and (q.loops == ql[:2]).all() and (q.vertices == qv[:3]).all()
        q = fp.advance_polygons(frame, 1.0, decode, 16, max_edges=int(oc[2]) - 1)  # more edges than the capacity: nothing
        assert list(q.counts) == [0, 0, 0, 0] and len(q.loops) == 0 and len(q.vertices) == 0


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    for hh, ww in ((48, 64), (61, 97)):
        frame = W.synth_frame(hh, ww, index=2)
        s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
        ref = S.simplify(*O.outline(s.klass), ww, 12)
        rl, rv, rc = ref
        k = s.stats.shape[0]
        d = Dev(ctx, bgr=frame.nbytes, loops=(len(rl) + 2) * 16, vertices=(len(rv) + 2) * 4, counts=16, stats=k * 64)
        try:
            d.put("bgr", frame)
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            P = d.ptr
            for stats in (True, False):
                d.poison("loops", "vertices", "counts", "stats")
                ctx.check(L.infur_frame_polygons_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 0, 0, 0, 12, P["loops"], len(rl) + 2, P["vertices"], len(rv) + 2,
                                                     P["counts"], P["stats"] if stats else None, k, None, C.byref(ow), C.byref(oh)))
                ctx.synchronize()
                assert (ow.value, oh.value) == (ww, hh)
                check_result(ref, (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32)))
                assert d.get("stats").tobytes() == s.stats.tobytes() if stats else (d.get("stats") == POISON).all()
        finally:
            d.free()


def test_fused_rules_and_error_codes(ctx, model):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    loops, verts = np.full((48 * 64, 4), 9, np.uint32), np.full(4 * 48 * 64, 9, np.uint32)
    stats, counts = np.zeros((21, 8), np.uint64), np.full(4, 77, np.uint32)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(lib=L, handle=h, decode=0, flags=0, skip=0, tol=16, lo=loops, ve=verts, count=counts, st=stats, st_cap=21, mode=0, factor=1.0, scaled=None):
        return lib.infur_frame_polygons(handle, p(frame), 64, 48, factor, mode, decode, flags, skip, 0, tol, p(lo), 48 * 64, p(ve), 4 * 48 * 64, p(count),
                                        p(st), st_cap, p(scaled), C.byref(ow), C.byref(oh))

    klass = FramePath(ctx).advance_segments(frame, 1.0, RAW).klass
    rl, rv, rc = S.simplify(*O.outline(klass), 64, 16)
    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48) and counts.tolist() == rc.tolist()
    assert (loops[:len(rl)] == rl).all() and (loops[len(rl):] == 9).all() and (verts[:len(rv)] == rv).all() and (verts[len(rv):] == 9).all()
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) == _lib.E_INVALID_ARG and call(tol=65536) == _lib.E_INVALID_ARG
    assert call(flags=4) == _lib.E_INVALID_ARG and call(flags=SKIP, skip=256) == _lib.E_INVALID_ARG
    assert call(lo=None, ve=None, count=None) == _lib.E_INVALID_ARG
    assert call(st_cap=20) == _lib.E_CAPACITY and call(st=None, st_cap=0) == _lib.OK
    assert call(factor=-1.0) == _lib.E_INVALID_SCALE
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_polygons(frame, 0.5, RAW, want_scaled=True)
        assert r.loops is None and r.vertices is None and r.counts is None and r.stats is None and r.scaled.shape == (24, 32, 3)
        assert (r.scaled == FramePath(c).advance_segments(frame, 0.5, RAW, want_scaled=True).scaled).all()
        loops[:] = 9
        counts[:] = 77
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED
        want_scaled = FramePath(c).advance_segments(frame, 1.0, RAW, want_scaled=True).scaled
        assert (scaled == want_scaled).all() and (loops == 9).all() and (counts == 77).all()


def test_polygon_calls_leave_the_cached_graphs_alone(blob50):
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
        for it in range(8):
            fr = frames[it % 4]
            args = (fr, 1.0, SOFTMAX if it & 1 else RAW, 11 + it, 0 if it & 2 else None, 8 if it & 1 else 4)
            s = fg.advance_polygons(*args, want_stats=bool(it & 4))
            e = fe.advance_polygons(*args)
            assert s.counts == e.counts and (s.loops == e.loops).all() and (s.vertices == e.vertices).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a polygons call caused a capture"
        assert cached1 >= cached0, "a polygons call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the polygons calls were not replayed"


# --------------------------------------------------------------------------- #
# 4. the command line
# --------------------------------------------------------------------------- #
def test_cli_round_trip(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip)]

    def cli(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]

    # the class plane beside its simplified outlines (0.7 px rounds to 11 sixteenths)
    recs = cli("--labels-out", str(tmp_path / "klass.u8"), "--outlines-out", str(tmp_path / "klass.outl"), "--outlines-tolerance", "0.7")
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    for i, (counts, loops, verts) in enumerate(TO.read_outlines_file(tmp_path / "klass.outl", 2)):
        rl, rv, rc = S.simplify(*O.outline(klass[i], CONN8), 128, 11)  # (8-connectivity is the command line's default)
        assert recs[i]["n_loops"] == rc[0] and recs[i]["n_degenerate"] == rc[2] and counts.tolist() == rc[:3].tolist()
        assert (loops == rl).all() and (verts == rv).all()
    # the fused call (no dense plane asked for), without the background class
    fused = cli("--outlines-out", str(tmp_path / "fused.outl"), "--outlines-skip", "0", "--connectivity", "4", "--outlines-tolerance", "1")
    for i, (counts, loops, verts) in enumerate(TO.read_outlines_file(tmp_path / "fused.outl", 2)):
        rl, rv, rc = S.simplify(*O.outline(klass[i], SKIP, 0), 128, 16)
        assert fused[i]["n_loops"] == rc[0] and counts.tolist() == rc[:3].tolist() and (loops == rl).all() and (verts == rv).all()
        assert fused[i]["classes"] == recs[i]["classes"]
    # per-object polygons from the label plane Regions left on the device
    lines = cli("--regions", "--min-pixels", "3", "--skip-background", "--outlines-skip", str(NONE), "--max-regions", str(96 * 128), "--regions-out",
                str(tmp_path / "labels.u32"), "--outlines-out", str(tmp_path / "labels.outl"), "--outlines-tolerance", "0.75")
    dense = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    for i, (counts, loops, verts) in enumerate(TO.read_outlines_file(tmp_path / "labels.outl", 2)):
        rl, rv, rc = S.simplify(*O.outline(dense[i], SKIP | CONN8, NONE), 128, 12)
        assert lines[i]["n_loops"] == rc[0] and counts.tolist() == rc[:3].tolist() and (loops == rl).all() and (verts == rv).all()
        assert sorted(outlines_by_value(loops, verts, 128)) == list(range(len(lines[i]["regions"])))
