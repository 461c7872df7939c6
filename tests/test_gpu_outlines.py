"""Outlines on the GPU: loop records, vertices and counts of ``infur_outlines*`` and of the fused ``infur_frame_outlines*``
against tests/outlines_ref.py.  Everything is an integer and a function of the plane alone, so every comparison is ``==`` on
whole arrays.  Every output buffer is filled with a poison byte first: what a call must leave alone still holds it afterwards,
and what it must write owes nothing to an initialisation."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import (Context, FramePath, Model, ModelCmd, Outlines, OutlinesCmd, OutlinesOut, outlines_by_value,
                                  outlines_polygons)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
SKIP, CONN8 = _lib.OUTLINES_SKIP, _lib.OUTLINES_CONN8
NONE = 0xFFFFFFFF
GUARD = 64
POISON = 0xA5
POISON32 = 0xA5A5A5A5


class Dev:
    """device buffers with GUARD poisoned bytes behind each; the whole buffer is poisoned when it is made"""

    def __init__(self, ctx, **sizes):
        self.ctx, self.sizes, self.ptr = ctx, sizes, {}
        for name, n in sizes.items():
            d = C.c_void_p(None)
            ctx.check(ctx.L.infur_dev_alloc(ctx.h, n + GUARD, C.byref(d)))
            self.ptr[name] = d
        self.poison()

    def poison(self, *names):
        for name in names or self.sizes:
            n = self.sizes[name] + GUARD
            buf = np.full(n, POISON, np.uint8)
            self.ctx.check(self.ctx.L.infur_memcpy_h2d(self.ctx.h, self.ptr[name], buf.ctypes.data, n))

    def put(self, name, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.sizes[name]
        if arr.nbytes:
            self.ctx.check(self.ctx.L.infur_memcpy_h2d(self.ctx.h, self.ptr[name], arr.ctypes.data, arr.nbytes))

    def get(self, name):
        """-> the buffer's bytes; asserts that the guard behind it is intact"""
        n = self.sizes[name]
        b = np.empty(n + GUARD, np.uint8)
        self.ctx.check(self.ctx.L.infur_memcpy_d2h(self.ctx.h, b.ctypes.data, self.ptr[name], n + GUARD))
        assert (b[n:] == POISON).all(), f"the guard bytes behind {name} were overwritten"
        return b[:n].copy()

    def free(self):
        for d in self.ptr.values():
            self.ctx.check(self.ctx.L.infur_dev_free(self.ctx.h, d))


def dev_outlines(ctx, plane, flags=0, skip_value=0, max_edges=0, loops_rows=0, vertex_rows=0, want=("loops", "vertices", "counts")):
    """infur_outlines_dev on poisoned device buffers -> (loops [loops_rows, 4] u32 and vertices [vertex_rows] u32 as the buffers
    hold them, counts [3]), None for what was not wanted (and that buffer is checked to be untouched)"""
    h, w = plane.shape
    d = Dev(ctx, plane=plane.nbytes, loops=loops_rows * 16, vertices=vertex_rows * 4, counts=12)
    try:
        d.put("plane", plane)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_outlines_dev(ctx.h, d.ptr["plane"], plane.dtype.itemsize, h, w, flags, skip_value, max_edges, p("loops"), loops_rows,
                                           p("vertices"), vertex_rows, p("counts")))
        ctx.synchronize()
        loops, vertices, counts = d.get("loops").view(np.uint32).reshape(loops_rows, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32)
        assert d.get("plane").tobytes() == plane.tobytes()  # the input is an input
        for name, got in (("loops", loops), ("vertices", vertices), ("counts", counts)):
            if name not in want:
                assert (got.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return (loops if "loops" in want else None, vertices if "vertices" in want else None, counts if "counts" in want else None)
    finally:
        d.free()


def check_result(ref, got, name=""):
    """whole arrays against the reference's; what lies behind the counts still holds the poison"""
    (rl, rv, rc), (loops, vertices, counts) = ref, got
    assert counts.tolist() == rc.tolist(), (name, counts, rc)
    assert (loops[:len(rl)] == rl).all() and (loops[len(rl):] == POISON32).all(), name
    assert (vertices[:len(rv)] == rv).all() and (vertices[len(rv):] == POISON32).all(), name


def check_against_reference(ctx, plane, flags=0, skip_value=0, name="", spare=7, max_edges=0):
    ref = O.outline(plane, flags, skip_value)
    rl, rv, rc = ref
    got = dev_outlines(ctx, plane, flags, skip_value, max_edges, loops_rows=len(rl) + spare, vertex_rows=len(rv) + spare)
    print(f"{name} {plane.shape[0]}x{plane.shape[1]} {plane.dtype} flags {flags} skip {skip_value}: {rc.tolist()}")
    check_result(ref, got, (name, plane.shape, flags, skip_value))
    return ref


def families(h, w):
    yield "smooth", R.smooth(h, w, seed=h + w)
    yield "noise2", R.noise(h, w, 2, seed=w)
    yield "noise21", R.noise(h, w, 21, seed=h)
    yield "single", R.single(h, w)
    yield "vstripes", R.stripes(h, w, vertical=True)
    yield "hstripes", R.stripes(h, w, vertical=False)
    yield "checkerboard", R.checkerboard(h, w)
    yield "staircase", R.staircase(h, w)
    yield "snake", O.snake(h, w)


def as_elem(klass, elem_bytes):
    return klass if elem_bytes == 1 else U.as_u32(klass)


SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (65, 130))


# --------------------------------------------------------------------------- #
# 1. infur_outlines_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conn", [0, CONN8])
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_families_equal_the_reference(ctx, elem_bytes, conn):
    assert ctx.L.infur_features() & _lib.FEATURE_OUTLINES  # (the first line: fails on a library without the feature)
    counts = {}
    for h, w in SHAPES:
        for name, k in families(h, w):
            plane = as_elem(k, elem_bytes)
            ref = check_against_reference(ctx, plane, conn, name=name)
            O.check_invariants(plane, conn, 0, *ref)
            counts[(name, h, w)] = ref[2].tolist()
            # skip on: the value of the first pixel and the value of the last pixel
            for skip_value in sorted({int(plane[0, 0]), int(plane[-1, -1])}):
                ref = check_against_reference(ctx, plane, conn | SKIP, skip_value, name=name)
                O.check_invariants(plane, conn | SKIP, skip_value, *ref)
    # what the families are for
    assert counts[("single", 65, 130)] == [1, 4, 2 * (65 + 130)] and counts[("single", 1, 1)] == [1, 4, 4]
    if conn:
        assert counts[("checkerboard", 65, 130)][2] == 4 * 65 * 130 and counts[("checkerboard", 65, 130)][0] < 65 * 130
    else:
        assert counts[("checkerboard", 65, 130)] == [65 * 130, 4 * 65 * 130, 4 * 65 * 130]  # every side of every pixel is an edge
    assert counts[("snake", 65, 130)][0] == 1 + 32  # the snake and the 32 strips of background between its coils
    if elem_bytes == 4:
        t = U.u32_table()
        assert t[0] == NONE and (t > (1 << 24)).sum() > 200  # the u32 planes do hold 0xFFFFFFFF and values a float would round


def test_the_snake_is_one_long_cycle():
    """(what the family is for; no device needed to say it) one cycle holds about half of all edges"""
    k = O.snake(65, 130)
    loops, vertices, counts = O.outline(k, SKIP, 0)
    assert counts[0] == 1 and counts[2] > 65 * 130 and loops[0, O.COUNT] == counts[1] > 120


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_cycles_that_span_workgroups_and_planes_of_one_row_or_column(ctx, elem_bytes):
    v = int(as_elem(R.single(1, 1), elem_bytes)[0, 0])
    # 6002 edges, one loop of 4 vertices: the cycle spans several workgroups of every launch
    rl, rv, rc = check_against_reference(ctx, as_elem(R.single(1, 3000), elem_bytes), name="single")
    assert rc.tolist() == [1, 4, 6002] and rl.tolist() == [[0, 4, v, 0]] and rv.tolist() == [0, 3000, 3001 + 3000, 3001]
    rl, rv, rc = check_against_reference(ctx, as_elem(R.single(3000, 1), elem_bytes), name="single")
    assert rc.tolist() == [1, 4, 6002] and rl.tolist() == [[0, 4, v, 0]] and rv.tolist() == [0, 1, 6001, 6000]
    check_against_reference(ctx, as_elem(R.noise(1, 3000, 2, seed=4), elem_bytes), SKIP | CONN8, int(as_elem(np.ones((1, 1), np.uint8), elem_bytes)[0, 0]), name="noise2")
    check_against_reference(ctx, as_elem(O.snake(40, 150), elem_bytes), SKIP, int(as_elem(np.zeros((1, 1), np.uint8), elem_bytes)[0, 0]), name="snake")


def test_more_than_1024_block_sums_single(ctx):
    """600 x 500 pixels are 1172 workgroups of the edge scan: the scan of the block sums takes a second pass"""
    h, w = 600, 500
    loops, vertices, counts = dev_outlines(ctx, R.single(h, w), loops_rows=3, vertex_rows=9)
    assert counts.tolist() == [1, 4, 2 * (h + w)]
    assert loops[0].tolist() == [0, 4, 3, 0] and (loops[1:] == POISON32).all()
    assert vertices[:4].tolist() == [0, w, h * (w + 1) + w, h * (w + 1)] and (vertices[4:] == POISON32).all()


def test_more_than_a_million_edges_checkerboard(ctx):
    """every side of every pixel is an edge: 1.2 M of them, so the loop scan takes its second pass too.  Under 4-connectivity
    every pixel is a loop of four vertices, in raster order"""
    h, w = 600, 500
    k = R.checkerboard(h, w)
    n = h * w
    loops, vertices, counts = dev_outlines(ctx, k, loops_rows=n + 3, vertex_rows=4 * n + 3)
    assert counts.tolist() == [n, 4 * n, 4 * n]
    i = np.arange(n, dtype=np.uint32)
    assert (loops[:n] == np.stack([4 * i, np.full(n, 4, np.uint32), k.reshape(-1).astype(np.uint32), 4 * i], axis=1)).all()
    x, y = i % w, i // w
    tl = y * (w + 1) + x  # N's tail (x, y), E's (x+1, y), S's (x+1, y+1), W's (x, y+1)
    assert (vertices[:4 * n].reshape(n, 4) == np.stack([tl, tl + 1, tl + w + 2, tl + w + 1], axis=1)).all()
    assert (loops[n:] == POISON32).all() and (vertices[4 * n:] == POISON32).all()
    # 8-connectivity, one colour skipped: the other colour is one region held together by its diagonals, every skipped pixel
    # off the border is a hole of four vertices in it, every edge is a corner edge; the rest through the invariants
    loops, vertices, counts = dev_outlines(ctx, k, SKIP | CONN8, 1, loops_rows=n, vertex_rows=2 * n)
    holes = (h - 2) * (w - 2) // 2
    assert counts.tolist() == [1 + holes, 2 * n, 2 * n]
    O.check_invariants_fast(k, SKIP | CONN8, 1, loops[:counts[0]], vertices, counts)
    assert (loops[counts[0]:] == POISON32).all() and int((loops[:counts[0], O.START] & 3 == 2).sum()) == holes


def test_capacity(ctx):
    for name, plane, flags, skip_value in (("smooth", R.smooth(33, 63), 0, 0), ("noise21", U.as_u32(R.noise(7, 65, 21)), SKIP | CONN8, int(U.u32_table()[3])),
                                           ("snake", O.snake(33, 63), SKIP, 0)):
        ref = O.outline(plane, flags, skip_value)
        rl, rv, rc = ref
        ne = int(rc[2])
        assert ne > 64 and ne & (ne - 1) and ne < 4 * plane.size
        rows = dict(loops_rows=len(rl) + 2, vertex_rows=len(rv) + 2)
        check_result(ref, dev_outlines(ctx, plane, flags, skip_value, 0, **rows), name)
        for cap in (ne, ne + 1, 3 * ne // 2 + 1, 4 * plane.size, 4 * plane.size + 9, NONE):  # exactly enough; not a power of two; beyond the worst case
            check_result(ref, dev_outlines(ctx, plane, flags, skip_value, cap, **rows), (name, cap))
        for cap in (ne - 1, ne // 2 + 1, 1):  # overflow: the edge count alone, everything else untouched
            loops, vertices, counts = dev_outlines(ctx, plane, flags, skip_value, cap, **rows)
            assert counts.tolist() == [0, 0, ne], (name, cap)
            assert (loops == POISON32).all() and (vertices == POISON32).all(), (name, cap)
            assert O.outline(plane, flags, skip_value, cap)[2].tolist() == [0, 0, ne]


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_truncation(ctx, elem_bytes):
    for name, k in (("smooth", R.smooth(65, 130)), ("noise21", R.noise(33, 63, 21)), ("checkerboard", R.checkerboard(7, 65))):
        plane = as_elem(k, elem_bytes)
        for flags, skip_value in ((0, 0), (SKIP | CONN8, int(plane[3, 3]))):
            rl, rv, rc = O.outline(plane, flags, skip_value)
            nl, nv = len(rl), len(rv)
            assert nl > 8 and nv > 8
            for lrows, vrows in ((0, nv), (1, nv), (nl - 1, nv), (nl, nv), (nl + 7, nv), (nl, 0), (nl, 1), (nl, nv - 1), (nl, nv + 7), (1, 1)):
                loops, vertices, counts = dev_outlines(ctx, plane, flags, skip_value, loops_rows=lrows, vertex_rows=vrows)
                assert counts.tolist() == rc.tolist(), (name, lrows, vrows)  # the full counts: that is how a caller sees truncation
                ml, mv = min(nl, lrows), min(nv, vrows)
                assert (loops[:ml] == rl[:ml]).all() and (loops[ml:] == POISON32).all(), (name, lrows, vrows)  # OFFSET is the full prefix sum
                assert (vertices[:mv] == rv[:mv]).all() and (vertices[mv:] == POISON32).all(), (name, lrows, vrows)


def test_calls_are_repeatable_and_contexts_agree(ctx):
    k = R.noise(65, 130, 3, seed=9)
    rl, rv, rc = O.outline(k, CONN8)
    rows = dict(loops_rows=len(rl), vertex_rows=len(rv))
    first = dev_outlines(ctx, k, CONN8, **rows)
    again = dev_outlines(ctx, k, CONN8, **rows)
    other = dev_outlines(ctx, R.smooth(135, 241), CONN8, **rows)  # another plane, a larger one, in between
    third = dev_outlines(ctx, k, CONN8, **rows)
    with Context(device=0) as c2:
        second_ctx = dev_outlines(c2, k, CONN8, **rows)
    check_result((rl, rv, rc), first)
    for run in (again, third, second_ctx):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run, first))
    assert other[2].tolist() != rc.tolist()


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_each_output_alone_equals_all_together(ctx, elem_bytes):
    for k in (R.smooth(33, 63), R.noise(7, 65, 3), R.noise(1, 5, 3)):
        plane = as_elem(k, elem_bytes)
        skip_value = int(plane[0, 0])
        rl, rv, rc = O.outline(plane, SKIP, skip_value)
        for want in (("loops",), ("vertices",), ("counts",), ("loops", "counts"), ("vertices", "counts"), ("loops", "vertices")):
            loops, vertices, counts = dev_outlines(ctx, plane, SKIP, skip_value, loops_rows=len(rl), vertex_rows=len(rv), want=want)
            assert loops is None or (loops == rl).all(), want
            assert vertices is None or (vertices == rv).all(), want
            assert counts is None or counts.tolist() == rc.tolist(), want
        # pointers with no rows are no tables
        loops, vertices, counts = dev_outlines(ctx, plane, SKIP, skip_value, loops_rows=0, vertex_rows=0)
        assert counts.tolist() == rc.tolist()


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    k = R.noise(6, 7, 3)
    d = Dev(ctx, plane=42 * 4, loops=16 * 50, vertices=4 * 200, counts=12)
    try:
        d.put("plane", U.as_u32(k))
        P = d.ptr
        call = lambda elem=4, flags=0, skip=0, hh=6, ww=7, pl=P["plane"], cap=0, lo=P["loops"], ve=P["vertices"], n=P["counts"]: L.infur_outlines_dev(  # noqa: E731
            h, pl, elem, hh, ww, flags, skip, cap, lo, 50, ve, 200, n)
        for elem in (0, 2, 3, 8):
            assert call(elem=elem) == _lib.E_INVALID_ARG
        assert call(flags=4) == _lib.E_INVALID_ARG and call(flags=7) == _lib.E_INVALID_ARG  # an unknown flag bit
        assert call(elem=1, flags=SKIP, skip=256) == _lib.E_INVALID_ARG and call(elem=1, skip=256) == _lib.E_INVALID_ARG
        assert call(lo=None, ve=None, n=None) == _lib.E_INVALID_ARG  # all outputs NULL
        assert "no output wanted" in ctx.last_error()
        assert L.infur_outlines_dev(h, P["plane"], 4, 6, 7, 0, 0, 0, P["loops"], 0, P["vertices"], 0, None) == _lib.E_INVALID_ARG  # tables without rows
        assert call(pl=None) == _lib.E_INVALID_ARG and "no plane pointer" in ctx.last_error()
        # 4*h*w must be below 2^32 - 1
        assert call(hh=32768, ww=32768) == _lib.E_INVALID_ARG and call(hh=0x40000000, ww=1) == _lib.E_INVALID_ARG and call(hh=65536, ww=65536) == _lib.E_INVALID_ARG
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("loops", "vertices", "counts"))  # no output is touched by a rejected call
        # an empty plane: counts = {0, 0, 0} and nothing else
        for hh, ww in ((0, 7), (6, 0), (0, 0)):
            d.poison("counts")
            assert call(hh=hh, ww=ww, pl=None) == _lib.OK
            ctx.synchronize()
            assert d.get("counts").view(np.uint32).tolist() == [0, 0, 0]
            assert (d.get("loops") == POISON).all() and (d.get("vertices") == POISON).all()
        assert call(hh=0, n=None) == _lib.OK and call(skip=256, flags=SKIP) == _lib.OK  # (a u32 plane may skip any u32)
        d.poison("counts")
        assert call(flags=CONN8) == _lib.OK
        ctx.synchronize()
        assert d.get("counts").view(np.uint32).tolist() == O.outline(U.as_u32(k), CONN8)[2].tolist()
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    counts = np.full(3, 77, np.uint32)
    loops = np.full((50, 4), 9, np.uint32)
    verts = np.full(200, 9, np.uint32)
    host = lambda elem=1, flags=0, skip=0, hh=6, ww=7, pl=k.ctypes.data, lo=loops.ctypes.data, ve=verts.ctypes.data, c=counts.ctypes.data: L.infur_outlines(  # noqa: E731
        h, pl, elem, hh, ww, flags, skip, 0, lo, 50, ve, 200, c)
    assert host(elem=2) == host(flags=4) == host(skip=300) == host(pl=None) == host(lo=None, ve=None, c=None) == _lib.E_INVALID_ARG
    assert host(hh=32768, ww=32768) == _lib.E_INVALID_ARG
    assert (counts == 77).all() and (loops == 9).all() and (verts == 9).all()
    assert host(hh=0) == _lib.OK and counts.tolist() == [0, 0, 0] and (loops == 9).all() and (verts == 9).all()
    with pytest.raises(Exception):
        Outlines(ctx).control(OutlinesCmd.Skip(-1))
    with pytest.raises(Exception):
        Outlines(ctx).control(OutlinesCmd.Connectivity(6))


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_host_pointer_call_and_processor(ctx, elem_bytes):
    proc = Outlines(ctx)
    assert proc.is_dirty()
    for k in (R.smooth(65, 130), R.noise(33, 63, 21), R.stripes(7, 65)):
        plane = as_elem(k, elem_bytes)
        hh, ww = plane.shape
        rl, rv, rc = O.outline(plane)
        nl, nv = len(rl), len(rv)
        out = OutlinesOut(loops_rows=nl + 5, vertex_rows=nv + 5)
        proc.control(OutlinesCmd.Skip(None)).control(OutlinesCmd.Connectivity(4)).advance(plane, out)
        assert not proc.is_dirty() and [out.n_loops, out.n_vertices, out.n_edges] == rc.tolist()
        assert out.loops.shape == (nl, 4) and (out.loops == rl).all() and (out.vertices == rv).all()
        # the helpers against the reference
        want = O.polygons(rl, rv, ww)
        got = outlines_polygons(out.loops, out.vertices, ww)
        assert len(got) == nl and all(g[0] == r[0] and g[1] == r[1] and g[2].dtype == np.int32 and g[2].tolist() == [list(p) for p in r[2]] for g, r in zip(got, want))
        by = outlines_by_value(out.loops, out.vertices, ww)
        assert sorted(by) == np.unique(plane).tolist()
        assert sum(len(g) for g in by.values()) == sum(not r[1] for r in want) and sum(len(g[1]) for v in by.values() for g in v) == sum(r[1] for r in want)
        # the caller's records and vertices beyond the counts, and beyond the rows, are left alone
        loops = np.full((nl + 2, 4), 7, np.uint32)
        verts = np.full(nv + 2, 7, np.uint32)
        counts = np.zeros(3, np.uint32)
        ctx.check(ctx.L.infur_outlines(ctx.h, plane.ctypes.data, elem_bytes, hh, ww, 0, 0, 0, loops.ctypes.data, nl + 2, verts.ctypes.data, nv + 2, counts.ctypes.data))
        assert counts.tolist() == rc.tolist() and (loops[:nl] == rl).all() and (loops[nl:] == 7).all() and (verts[:nv] == rv).all() and (verts[nv:] == 7).all()
        loops[:] = 7
        verts[:] = 7
        ctx.check(ctx.L.infur_outlines(ctx.h, plane.ctypes.data, elem_bytes, hh, ww, 0, 0, 0, loops.ctypes.data, 1, verts.ctypes.data, 3, counts.ctypes.data))
        assert counts.tolist() == rc.tolist() and (loops[0] == rl[0]).all() and (loops[1:] == 7).all() and (verts[:3] == rv[:3]).all() and (verts[3:] == 7).all()
        # an edge capacity that is too small, through the host-pointer call: the edge count alone
        ctx.check(ctx.L.infur_outlines(ctx.h, plane.ctypes.data, elem_bytes, hh, ww, 0, 0, int(rc[2]) - 1, loops.ctypes.data, 1, verts.ctypes.data, 3, counts.ctypes.data))
        assert counts.tolist() == [0, 0, int(rc[2])] and (loops[1:] == 7).all() and (verts[3:] == 7).all()
        # skip and 8-connectivity, through the processor, with truncated tables
        skip_value = int(plane[hh // 2, ww // 2])
        sl, sv, sc = O.outline(plane, SKIP | CONN8, skip_value)
        out = OutlinesOut(loops_rows=2, vertex_rows=5)
        proc.control(OutlinesCmd.Skip(skip_value)).control(OutlinesCmd.Connectivity(8))
        assert proc.is_dirty()
        proc.advance(plane, out)
        assert [out.n_loops, out.n_vertices, out.n_edges] == sc.tolist() and (out.loops == sl[:2]).all() and (out.vertices == sv[:5]).all()
        whole = [int(off + cnt) <= 5 for off, cnt in sl[:2, :2].tolist()]  # a loop whose vertices were cut off ends the list
        assert len(outlines_polygons(out.loops, out.vertices, ww)) == (2 if all(whole) else 1 if whole[0] else 0)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_composition_with_regions_on_the_device(ctx, connectivity):
    """infur_regions_dev, then infur_outlines_dev on the label plane it left on the device: per-object polygons, no dense plane
    to the host"""
    k = R.smooth(65, 130)
    h, w = k.shape
    rflags, min_pixels = _lib.REGIONS_SKIP_BACKGROUND, 6
    labels, table, n_reg = R.label(k, None, connectivity, min_pixels, rflags)
    assert (labels == NONE).any() and n_reg > 3
    flags = SKIP | (CONN8 if connectivity == 8 else 0)
    ref = O.outline(labels, flags, NONE)
    rl, rv, rc = ref
    d = Dev(ctx, klass=h * w, labels=h * w * 4, loops=(len(rl) + 3) * 16, vertices=(len(rv) + 3) * 4, counts=12)
    try:
        d.put("klass", k)
        P = d.ptr
        ctx.check(ctx.L.infur_regions_dev(ctx.h, P["klass"], None, h, w, connectivity, min_pixels, rflags, P["labels"], None, 0, None))
        ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["labels"], 4, h, w, flags, NONE, 0, P["loops"], len(rl) + 3, P["vertices"], len(rv) + 3, P["counts"]))
        ctx.synchronize()
        assert (d.get("labels").view(np.uint32).reshape(h, w) == labels).all()
        got = (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
        check_result(ref, got)
        # for every region, the smallest START >> 2 among its outer loops is its first pixel
        loops = got[0][:len(rl)]
        O.check_invariants(labels, flags, NONE, loops, got[1][:len(rv)], got[2], first_of_label={i: int(table[i, R.FIRST]) for i in range(n_reg)})
        by = outlines_by_value(loops, got[1], w)  # one object's polygon with its holes
        assert sorted(by) == list(range(n_reg))
        if connectivity == 8:
            assert all(len(g) == 1 for g in by.values())  # one outer loop per region
    finally:
        d.free()


# --------------------------------------------------------------------------- #
# 2. the fused frame path
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_segments_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    for (h, w), factor in (((61, 97), 1.0), ((120, 160), 1.0), ((120, 160), 0.5)):
        frame = W.synth_frame(h, w, index=h)
        s = fp.advance_segments(frame, factor, decode)
        oh, ow = s.klass.shape
        rl, rv, rc = O.outline(s.klass)
        r = fp.advance_outlines(frame, factor, decode, loops_rows=len(rl) + 1, vertex_rows=len(rv) + 1, want_scaled=True)
        assert list(r.counts) == rc.tolist() and (r.loops == rl).all() and (r.vertices == rv).all() and r.shape == (oh, ow), (h, w, factor)
        assert r.stats.tobytes() == s.stats.tobytes()  # captions come with the polygons
        assert r.scaled.shape == (oh, ow, 3)
        lo, _ = model.lowres()  # infur_model_read_lowres still works afterwards
        assert lo.size > 0 and np.isfinite(lo).all()
        # skip, 8-connectivity and truncated tables; no statistics
        skip_value = int(s.klass[0, 0])
        sl, sv, sc = O.outline(s.klass, SKIP | CONN8, skip_value)
        q = fp.advance_outlines(frame, factor, decode, skip=skip_value, connectivity=8, loops_rows=2, vertex_rows=3, want_stats=False)
        assert list(q.counts) == sc.tolist() and q.stats is None and (q.loops == sl[:2]).all() and (q.vertices == sv[:3]).all()
        q = fp.advance_outlines(frame, factor, decode, max_edges=int(rc[2]) - 1)
        assert list(q.counts) == [0, 0, int(rc[2])] and len(q.loops) == 0 and len(q.vertices) == 0


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    for hh, ww in ((52, 100), (50, 99)):
        frame = W.synth_frame(hh, ww, index=2)
        s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
        ref = O.outline(s.klass)
        rl, rv, rc = ref
        k = s.stats.shape[0]
        d = Dev(ctx, bgr=frame.nbytes, loops=(len(rl) + 2) * 16, vertices=(len(rv) + 2) * 4, counts=12, stats=k * 64)
        try:
            d.put("bgr", frame)
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            P = d.ptr
            for stats in (True, False):
                d.poison("loops", "vertices", "counts", "stats")
                ctx.check(L.infur_frame_outlines_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 0, 0, 0, P["loops"], len(rl) + 2, P["vertices"], len(rv) + 2,
                                                     P["counts"], P["stats"] if stats else None, k, None, C.byref(ow), C.byref(oh)))
                ctx.synchronize()
                assert (ow.value, oh.value) == (ww, hh)
                check_result(ref, (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32)))
                if stats:
                    assert d.get("stats").tobytes() == s.stats.tobytes()
                else:
                    assert (d.get("stats") == POISON).all()
        finally:
            d.free()


def test_fused_rules_and_error_codes(ctx, model):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    loops = np.full((48 * 64, 4), 9, np.uint32)
    verts = np.full(4 * 48 * 64, 9, np.uint32)
    stats = np.zeros((21, 8), np.uint64)
    counts = np.full(3, 77, np.uint32)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(lib=L, handle=h, decode=0, flags=0, skip=0, lo=loops, ve=verts, count=counts, st=stats, st_cap=21, mode=0, factor=1.0, scaled=None):
        return lib.infur_frame_outlines(handle, p(frame), 64, 48, factor, mode, decode, flags, skip, 0, p(lo), 48 * 64, p(ve), 4 * 48 * 64, p(count), p(st),
                                        st_cap, p(scaled), C.byref(ow), C.byref(oh))

    klass = FramePath(ctx).advance_segments(frame, 1.0, RAW).klass
    rl, rv, rc = O.outline(klass)
    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48) and counts.tolist() == rc.tolist()
    assert (loops[:len(rl)] == rl).all() and (loops[len(rl):] == 9).all() and (verts[:len(rv)] == rv).all() and (verts[len(rv):] == 9).all()
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) == _lib.E_INVALID_ARG
    assert call(flags=4) == _lib.E_INVALID_ARG and call(flags=SKIP, skip=256) == _lib.E_INVALID_ARG
    assert call(lo=None, ve=None, count=None) == _lib.E_INVALID_ARG
    assert call(st_cap=20) == _lib.E_CAPACITY and call(st=None, st_cap=0) == _lib.OK
    assert call(factor=-1.0) == _lib.E_INVALID_SCALE
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_outlines(frame, 0.5, RAW, want_scaled=True)
        assert r.loops is None and r.vertices is None and r.counts is None and r.stats is None and r.scaled.shape == (24, 32, 3)
        assert (r.scaled == FramePath(c).advance_segments(frame, 0.5, RAW, want_scaled=True).scaled).all()
        loops[:] = 9
        counts[:] = 77
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED
        want_scaled = FramePath(c).advance_segments(frame, 1.0, RAW, want_scaled=True).scaled
        assert (scaled == want_scaled).all() and (loops == 9).all() and (counts == 77).all()


def test_outlines_calls_leave_the_cached_graphs_alone(blob50):
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
            args = (fr, 1.0, SOFTMAX if it & 1 else RAW, 0 if it & 2 else None, 8 if it & 1 else 4)
            s = fg.advance_outlines(*args, want_stats=bool(it & 4))
            e = fe.advance_outlines(*args)
            assert s.counts == e.counts and (s.loops == e.loops).all() and (s.vertices == e.vertices).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "an outlines call caused a capture"
        assert cached1 >= cached0, "an outlines call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the outlines calls were not replayed"


# --------------------------------------------------------------------------- #
# 3. the command line
# --------------------------------------------------------------------------- #
def read_outlines_file(path, frames):
    """-> [(counts [3], loops [n_loops, 4], vertices [n_vertices])] of an --outlines-out file, which must hold exactly `frames` frames"""
    words = np.frombuffer(open(path, "rb").read(), np.uint32)
    out, at = [], 0
    for _ in range(frames):
        nl, nv = int(words[at]), int(words[at + 1])
        out.append((words[at:at + 3], words[at + 3:at + 3 + 4 * nl].reshape(nl, 4), words[at + 3 + 4 * nl:at + 3 + 4 * nl + nv]))
        at += 3 + 4 * nl + nv
    assert at == len(words)
    return out


def test_cli_round_trip(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip)]

    def cli(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]

    # the class plane beside its outlines
    recs = cli("--labels-out", str(tmp_path / "klass.u8"), "--outlines-out", str(tmp_path / "klass.outl"))
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    for i, (counts, loops, verts) in enumerate(read_outlines_file(tmp_path / "klass.outl", 2)):
        rl, rv, rc = O.outline(klass[i], CONN8)  # (8-connectivity is the command line's default)
        assert recs[i]["n_loops"] == rc[0] and counts.tolist() == rc.tolist() and (loops == rl).all() and (verts == rv).all()
    # the fused call (no dense plane asked for), without the background class: the same captions
    fused = cli("--outlines-out", str(tmp_path / "fused.outl"), "--outlines-skip", "0", "--connectivity", "4")
    for i, (counts, loops, verts) in enumerate(read_outlines_file(tmp_path / "fused.outl", 2)):
        rl, rv, rc = O.outline(klass[i], SKIP, 0)
        assert fused[i]["n_loops"] == rc[0] and counts.tolist() == rc.tolist() and (loops == rl).all() and (verts == rv).all()
        assert fused[i]["classes"] == recs[i]["classes"]
    # per-object polygons from the label plane Regions left on the device
    common = ("--regions", "--min-pixels", "3", "--skip-background", "--outlines-skip", str(NONE), "--max-regions", str(96 * 128))
    lines = cli(*common, "--regions-out", str(tmp_path / "labels.u32"), "--outlines-out", str(tmp_path / "labels.outl"))
    dense = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    for i, (counts, loops, verts) in enumerate(read_outlines_file(tmp_path / "labels.outl", 2)):
        rl, rv, rc = O.outline(dense[i], SKIP | CONN8, NONE)
        assert lines[i]["n_loops"] == rc[0] and counts.tolist() == rc.tolist() and (loops == rl).all() and (verts == rv).all()
        assert sorted(outlines_by_value(loops, verts, 128)) == list(range(len(lines[i]["regions"])))
