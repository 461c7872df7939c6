"""Anchors on the GPU: the squared distances and the anchor rows of ``infur_anchors*`` and of the fused ``infur_frame_anchors*``
against tests/anchors_ref.py.  Everything is an integer, exact and a function of the plane alone, so every comparison is ``==``
on whole arrays.  Every output buffer is filled with a poison byte first: what a call must leave alone still holds it
afterwards, and what it must write owes nothing to an initialisation."""
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
from infur_amd.processors import Anchors, AnchorsCmd, AnchorsOut, Context, FramePath, Model, ModelCmd, region_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchors_ref as A  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
SKIP = _lib.ANCHORS_SKIP
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


def dev_anchors(ctx, plane, flags=0, skip_value=0, rows=0, want=("dist2", "anchors")):
    """infur_anchors_dev on poisoned device buffers -> (dist2 [h, w] u32, anchors [rows, 2] u32), None for what was not wanted
    (and that buffer is checked to be untouched)"""
    h, w = plane.shape
    d = Dev(ctx, plane=plane.nbytes, dist2=h * w * 4, anchors=rows * 8)
    try:
        d.put("plane", plane)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_anchors_dev(ctx.h, d.ptr["plane"], plane.dtype.itemsize, h, w, flags, skip_value, p("dist2"), p("anchors"), rows))
        ctx.synchronize()
        dist2, anchors = d.get("dist2").view(np.uint32).reshape(h, w), d.get("anchors").view(np.uint32).reshape(rows, 2)
        assert d.get("plane").tobytes() == plane.tobytes()  # the input is an input
        for name, got in (("dist2", dist2), ("anchors", anchors)):
            if name not in want:
                assert (got.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return dist2 if "dist2" in want else None, anchors if "anchors" in want else None
    finally:
        d.free()


@functools.lru_cache(maxsize=None)
def _reference(key):
    plane, flags, skip_value, rows = _PLANES[key[0]], key[1], key[2], key[3]
    d = A.distance(plane, flags, skip_value)
    d.setflags(write=False)
    return d, A.anchors(plane, d, rows)


_PLANES = {}


def reference(plane, flags, skip_value, rows):
    """the reference's answer, computed once per (plane, flags, skip_value, rows) and left unchanged"""
    key = (plane.shape, plane.dtype.str, plane.tobytes())
    _PLANES.setdefault(key, plane)
    return _reference((key, flags, skip_value, rows))


def check_against_reference(ctx, plane, flags=0, skip_value=0, rows=22, name=""):
    rd, ra = reference(plane, flags, skip_value, rows)
    dist2, anchors = dev_anchors(ctx, plane, flags, skip_value, rows=rows)
    print(f"{name} {plane.shape[0]}x{plane.shape[1]} {plane.dtype} flags {flags} skip {skip_value}: largest dist2 {int(rd.max()) if rd.size else 0}")
    assert (dist2 == rd).all(), (name, plane.shape, plane.dtype, flags, skip_value)
    assert (anchors == ra).all(), (name, plane.shape, plane.dtype, flags, skip_value)
    return rd, ra


def families(h, w):
    yield "smooth", R.smooth(h, w, seed=h + w)
    yield "noise2", R.noise(h, w, 2, seed=w)
    yield "noise21", R.noise(h, w, 21, seed=h)
    yield "single", R.single(h, w)
    yield "vstripes", R.stripes(h, w, vertical=True)
    yield "hstripes", R.stripes(h, w, vertical=False)
    yield "checkerboard", R.checkerboard(h, w)
    yield "staircase", R.staircase(h, w)
    yield "disc", A.disc(h, w)
    yield "annulus", A.disc(h, w, annulus=True)
    if h >= 16 and w >= 16:
        yield "c", A.letter_c(h, w)


def as_elem(klass, elem_bytes):
    return klass if elem_bytes == 1 else U.as_u32(klass)


# (the kernels pick no form by size: the last two shapes make the per-row loops over 64-column tiles take more than one pass --
#  258 tiles for the 256 threads that walk the tile ends, and more than four tiles per wave)
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (135, 241), (300, 3), (2, 16500))


# --------------------------------------------------------------------------- #
# 1. infur_anchors_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_families_equal_the_reference(ctx, elem_bytes):
    assert ctx.L.infur_features() & _lib.FEATURE_ANCHORS  # (the first line: fails on a library without the feature)
    largest = {}
    for h, w in SHAPES:
        for name, k in families(h, w):
            plane = as_elem(k, elem_bytes)
            largest[(name, h, w)] = int(check_against_reference(ctx, plane, name=name)[0].max())
            # skip on: the value of the first pixel, of the last pixel, and for u32 the one that stands for "no region"
            for skip_value in sorted({int(plane[0, 0]), int(plane[-1, -1])} | ({NONE} if elem_bytes == 4 else set())):
                rd, _ = check_against_reference(ctx, plane, SKIP, skip_value, name=name)
                assert ((rd == 0) == (plane == skip_value)).all()
    # what the shapes are for
    assert largest[("single", 135, 241)] == 68 * 68  # through a run of four waves
    assert largest[("single", 300, 3)] == 4 and largest[("vstripes", 300, 3)] == 1  # a tall column walk
    assert largest[("single", 2, 16500)] == 1 == largest[("single", 1, 1)] and largest[("hstripes", 2, 16500)] == 1
    assert largest[("checkerboard", 135, 241)] == 1 and largest[("disc", 135, 241)] > 50 * 50
    if elem_bytes == 4:
        t = U.u32_table()
        assert t[0] == NONE and (t > (1 << 24)).sum() > 200  # the u32 planes do hold 0xFFFFFFFF and values a float would round


def test_the_letter_c(ctx):
    c = A.letter_c()
    dist2, anchors = dev_anchors(ctx, c, SKIP, 0, rows=3)
    assert anchors.tolist() == [[NONE, 0], [100, 9], [NONE, 0]] and c[4, 4] == 1 and dist2[4, 4] == 9
    ys, xs = np.nonzero(c == 1)
    assert c[int(ys.mean()), int(xs.mean())] == 0  # where the centroid would have put the caption


@pytest.mark.parametrize("shape", [(1, 65535), (65535, 1), (3, 40000)])
def test_the_longest_sides(ctx, shape):
    """the row distance is a u16 and reaches 32768 in a row of 65535; a column of 65535 is that many workgroups"""
    h, w = shape
    rd, ra = check_against_reference(ctx, R.single(h, w), rows=4, name="single")
    assert int(rd.max()) == (4 if h == 3 else 1) and ra[3].tolist() == [w + 1 if h == 3 else 0, int(rd.max())]
    k = R.single(h, w)
    k[h // 2, w // 2:] = 1  # a break in the middle: the runs to its left and right end there
    check_against_reference(ctx, k, SKIP, 1, rows=4, name="single with a break")
    if h == 1:
        line = R.single(1, w)
        line[0, 0] = 0
        dist2, anchors = dev_anchors(ctx, line, SKIP, 0, rows=4, want=("anchors",))
        assert anchors[3].tolist() == [1, 1]  # a row of height 1: every pixel touches the frame, the first one wins


# --------------------------------------------------------------------------- #
# 2. rows, untouched memory, determinism, capture
# --------------------------------------------------------------------------- #
def test_rows_below_equal_and_above_the_number_of_values(ctx):
    k = R.smooth(135, 241)
    labels, _, n = R.label(k, None, 8, min_pixels=20, flags=1)
    assert n > 8 and (labels == NONE).any()
    for plane, top in ((k, int(k.max()) + 1), (labels, n)):
        full_d, full_a = reference(plane, SKIP, NONE if plane.dtype == np.uint32 else 0, top + 9)
        assert (full_a[top:, 0] == NONE).all() and (full_a[top:, 1] == 0).all()
        for rows in (1, top - 1, top, top + 9):
            dist2, anchors = dev_anchors(ctx, plane, SKIP, NONE if plane.dtype == np.uint32 else 0, rows=rows)
            assert (dist2 == full_d).all(), rows  # a pixel whose value is at or above rows still gets its distance
            assert (anchors == full_a[:rows]).all(), rows  # rows without a pixel hold NONE: every row is written
    # each anchor pixel carries its row's value
    _, anchors = dev_anchors(ctx, labels, SKIP, NONE, rows=n)
    assert (labels.ravel()[anchors[:, 0]] == np.arange(n)).all()


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_each_output_alone_equals_both_together(ctx, elem_bytes):
    for k in (R.smooth(135, 241), R.noise(7, 65, 3), R.noise(1, 5, 3)):
        plane = as_elem(k, elem_bytes)
        skip_value = int(plane[0, 0])
        rd, ra = reference(plane, SKIP, skip_value, 9)
        dist2, anchors = dev_anchors(ctx, plane, SKIP, skip_value, rows=9, want=("dist2",))
        assert anchors is None and (dist2 == rd).all()
        dist2, anchors = dev_anchors(ctx, plane, SKIP, skip_value, rows=9, want=("anchors",))
        assert dist2 is None and (anchors == ra).all()
        dist2, anchors = dev_anchors(ctx, plane, SKIP, skip_value, rows=0)  # a table pointer with no rows is no table
        assert (dist2 == rd).all() and anchors.size == 0


def test_calls_are_repeatable_and_contexts_agree(ctx):
    k = R.noise(135, 241, 3, seed=9)  # three classes: thousands of atomic maxima per row of the table
    first = dev_anchors(ctx, k, rows=5)
    again = dev_anchors(ctx, k, rows=5)
    other = dev_anchors(ctx, R.smooth(270, 480), rows=5)  # another plane, a larger one, in between: the scratch grows
    third = dev_anchors(ctx, k, rows=5)
    with Context(device=0) as c2:
        second_ctx = dev_anchors(c2, k, rows=5)
    for run in (again, third, second_ctx):
        assert run[0].tobytes() == first[0].tobytes() and run[1].tobytes() == first[1].tobytes()
    assert other[0].shape != first[0].shape and (other[0] == A.distance(R.smooth(270, 480))).all()
    assert (first[0] == reference(k, 0, 0, 5)[0]).all() and (first[1] == reference(k, 0, 0, 5)[1]).all()


def _hip():
    """the HIP runtime this process already runs on (the one mapped file, not a second copy)"""
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [C.c_void_p]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


def test_the_device_call_inside_a_captured_graph(ctx):
    """after one call outside the capture the scratch is there: the call is a memset and three launches, and a graph of them
    replays to the same bytes on whatever plane lies in the input buffer"""
    hip = _hip()
    h, w, rows = 33, 63, 9
    first, second = R.smooth(h, w, seed=3), R.noise(h, w, 3, seed=5)
    d = Dev(ctx, plane=h * w, dist2=h * w * 4, anchors=rows * 8)
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    try:
        P, stream = d.ptr, C.c_void_p(ctx.stream)
        call = lambda: ctx.L.infur_anchors_dev(ctx.h, P["plane"], 1, h, w, SKIP, 0, P["dist2"], P["anchors"], rows)  # noqa: E731
        d.put("plane", first)
        ctx.check(call())  # the warm call
        ctx.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for plane in (second, first):
            d.poison("dist2", "anchors")
            d.put("plane", plane)
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            rd, ra = reference(plane, SKIP, 0, rows)
            assert (d.get("dist2").view(np.uint32).reshape(h, w) == rd).all() and (d.get("anchors").view(np.uint32).reshape(rows, 2) == ra).all()
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    k = R.noise(6, 7, 3)
    d = Dev(ctx, plane=42 * 4, dist2=42 * 4, anchors=8 * 5)
    try:
        d.put("plane", U.as_u32(k))
        P = d.ptr
        call = lambda elem=4, flags=0, skip=0, hh=6, ww=7, pl=P["plane"], dist2=P["dist2"], anchors=P["anchors"], rows=5: L.infur_anchors_dev(  # noqa: E731
            h, pl, elem, hh, ww, flags, skip, dist2, anchors, rows)
        for elem in (0, 2, 3, 8):
            assert call(elem=elem) == _lib.E_INVALID_ARG and "elem_bytes" in ctx.last_error()
        assert call(flags=2) == _lib.E_INVALID_ARG and call(flags=3) == _lib.E_INVALID_ARG and "unknown anchors flags" in ctx.last_error()
        assert call(elem=1, flags=SKIP, skip=256) == _lib.E_INVALID_ARG and call(elem=1, skip=256) == _lib.E_INVALID_ARG and "skip_value" in ctx.last_error()
        assert call(hh=65536) == _lib.E_INVALID_ARG and call(ww=65536) == _lib.E_INVALID_ARG and "up to 65535" in ctx.last_error()
        assert call(dist2=None, anchors=None) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()
        assert call(dist2=None, rows=0) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()  # a table without rows: not wanted
        assert call(pl=None) == _lib.E_INVALID_ARG and "no plane pointer" in ctx.last_error()
        # the order of the checks, as Runs and Outlines make them: element size, flags, skip value, sides, wanted, plane
        assert call(elem=2, flags=2, hh=65536, pl=None, dist2=None, anchors=None) == _lib.E_INVALID_ARG and "elem_bytes" in ctx.last_error()
        assert call(elem=1, flags=2, skip=256, hh=65536, pl=None, dist2=None, anchors=None) == _lib.E_INVALID_ARG and "flags" in ctx.last_error()
        assert call(elem=1, skip=256, hh=65536, pl=None, dist2=None, anchors=None) == _lib.E_INVALID_ARG and "skip_value" in ctx.last_error()
        assert call(hh=65536, pl=None, dist2=None, anchors=None) == _lib.E_INVALID_ARG and "up to 65535" in ctx.last_error()
        assert call(pl=None, dist2=None, anchors=None) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("dist2", "anchors"))  # no output is touched by a rejected call
        # an empty plane: the NONE rows and nothing else
        for hh, ww in ((0, 7), (6, 0), (0, 0)):
            d.poison("dist2", "anchors")
            assert call(hh=hh, ww=ww, pl=None) == _lib.OK
            ctx.synchronize()
            assert d.get("anchors").view(np.uint32).reshape(5, 2).tolist() == [[NONE, 0]] * 5 and (d.get("dist2") == POISON).all()
        assert call(hh=0, anchors=None) == _lib.OK and call(skip=256, flags=SKIP) == _lib.OK  # (a u32 plane may skip any u32)
        d.poison("dist2", "anchors")
        assert call(rows=3) == _lib.OK
        ctx.synchronize()
        got = d.get("anchors").view(np.uint32)
        assert (got[:6].reshape(3, 2) == reference(U.as_u32(k), 0, 0, 3)[1]).all() and (got[6:] == POISON32).all()  # rows beyond `rows` are the caller's
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    dist2 = np.full((6, 7), 9, np.uint32)
    anchors = np.full((5, 2), 9, np.uint32)
    host = lambda elem=1, flags=0, skip=0, hh=6, ww=7, pl=k.ctypes.data, d2=dist2.ctypes.data, a=anchors.ctypes.data, rows=5: L.infur_anchors(  # noqa: E731
        h, pl, elem, hh, ww, flags, skip, d2, a, rows)
    assert host(elem=2) == host(flags=4) == host(skip=300) == host(pl=None) == host(d2=None, a=None) == host(d2=None, rows=0) == _lib.E_INVALID_ARG
    assert host(hh=65536) == host(ww=65536) == _lib.E_INVALID_ARG
    assert (dist2 == 9).all() and (anchors == 9).all()
    assert host(hh=0) == _lib.OK and (dist2 == 9).all() and anchors.tolist() == [[NONE, 0]] * 5
    anchors[:] = 9
    assert host(ww=0, rows=2) == _lib.OK and anchors.tolist() == [[NONE, 0]] * 2 + [[9, 9]] * 3
    with pytest.raises(Exception):
        Anchors(ctx).control(AnchorsCmd.Skip(-1))


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_host_pointer_call_and_processor(ctx, elem_bytes):
    proc = Anchors(ctx)
    assert proc.is_dirty()
    for k in (R.smooth(135, 241), R.noise(33, 63, 21), A.disc(7, 65), A.letter_c()):
        plane = as_elem(k, elem_bytes)
        rd, ra = reference(plane, 0, 0, 22)
        out = AnchorsOut(rows=22)
        proc.control(AnchorsCmd.Skip(None)).advance(plane, out)
        assert not proc.is_dirty() and (out.dist2 == rd).all() and (out.anchors == ra).all()
        skip_value = int(plane[plane.shape[0] // 2, plane.shape[1] // 2])
        sd, sa = reference(plane, SKIP, skip_value, 4)
        out = AnchorsOut(rows=4, want_dist2=False)
        proc.control(AnchorsCmd.Skip(skip_value))
        assert proc.is_dirty()
        proc.advance(plane, out)
        assert out.dist2 is None and (out.anchors == sa).all()
        out = AnchorsOut(rows=0)
        proc.advance(plane, out)
        assert out.anchors is None and (out.dist2 == sd).all()


# --------------------------------------------------------------------------- #
# 3. the fused frame path
# --------------------------------------------------------------------------- #
FRAME_H, FRAME_W = 96, 128


@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_regions_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    frame = W.synth_frame(FRAME_H, FRAME_W, index=5)
    for factor, kw in ((1.0, dict(min_pixels=3, flags=_lib.REGIONS_SKIP_BACKGROUND)), (0.5, dict(connectivity=4))):
        r = fp.advance_regions(frame, factor, decode, table_rows=4096, **kw)
        a = fp.advance_anchors(frame, factor, decode, table_rows=4096, want_scaled=True, **kw)
        assert a.n == r.n > 1 and (a.labels == r.labels).all() and (a.table == r.table).all() and (a.klass == r.klass).all() and (a.conf == r.conf).all()
        rd, ra = reference(r.labels, SKIP, NONE, r.n)
        assert (a.dist2 == rd).all() and (a.anchors == ra).all(), factor
        assert (r.labels.ravel()[a.anchors[:, 0]] == np.arange(r.n)).all()  # row i's anchor pixel carries label i
        assert a.scaled.shape == r.labels.shape + (3,)
        # a truncated table, nothing else wanted: the label plane goes to the library's own scratch
        q = fp.advance_anchors(frame, factor, decode, table_rows=2, want_labels=False, want_klass=False, want_conf=False, want_dist2=False, **kw)
        assert q.n == r.n and q.labels is None and q.dist2 is None and (q.anchors == ra[:2]).all() and (q.table == r.table[:2]).all()
        recs = region_summary(a.table, a.n, a.labels.shape[1], a.labels.shape[0], anchors=a.anchors)
        assert all(r.labels[rec["anchor"][1], rec["anchor"][0]] == rec["id"] and rec["radius"] >= 1.0 for rec in recs)
        lo, _ = model.lowres()  # infur_model_read_lowres still works afterwards
        assert lo.size > 0 and np.isfinite(lo).all()


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    hh, ww = FRAME_H, FRAME_W
    frame = W.synth_frame(hh, ww, index=2)
    r = FramePath(ctx).advance_regions(frame, 1.0, SOFTMAX, table_rows=hh * ww)
    rows = r.n + 3
    rd, ra = reference(r.labels, SKIP, NONE, rows)
    d = Dev(ctx, bgr=frame.nbytes, labels=hh * ww * 4, table=rows * 80, n=4, dist2=hh * ww * 4, anchors=rows * 8)
    try:
        d.put("bgr", frame)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        P = d.ptr
        for want in (("labels", "table", "n", "dist2", "anchors"), ("dist2",), ("anchors",), ("labels", "n")):
            d.poison("labels", "table", "n", "dist2", "anchors")
            p = lambda name: P[name] if name in want else None  # noqa: E731
            ctx.check(L.infur_frame_anchors_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 8, 0, 0, None, None, 0, p("labels"), hh * ww * 4, p("table"), rows,
                                                p("n"), None, C.byref(ow), C.byref(oh), p("dist2"), hh * ww * 4, p("anchors")))
            ctx.synchronize()
            assert (ow.value, oh.value) == (ww, hh)
            got = {name: d.get(name) for name in ("labels", "table", "n", "dist2", "anchors")}
            for name in got:
                if name not in want:
                    assert (got[name] == POISON).all(), (want, name)
            if "labels" in want:
                assert (got["labels"].view(np.uint32).reshape(hh, ww) == r.labels).all() and got["n"].view(np.uint32)[0] == r.n
            if "table" in want:
                t = got["table"].view(np.uint64).reshape(rows, 10)
                assert (t[:r.n] == r.table).all() and (t[r.n:].view(np.uint8) == POISON).all()
            if "dist2" in want:
                assert (got["dist2"].view(np.uint32).reshape(hh, ww) == rd).all()
            if "anchors" in want:
                assert (got["anchors"].view(np.uint32).reshape(rows, 2) == ra).all()  # every one of the rows, NONE beyond n
    finally:
        d.free()


def test_fused_rules_and_error_codes(ctx, model):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    npix = 48 * 64
    labels, dist2 = np.full((48, 64), 9, np.uint32), np.full((48, 64), 9, np.uint32)
    table, anchors = np.zeros((64, 10), np.uint64), np.full((64, 2), 9, np.uint32)
    n, ow, oh = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(fn="infur_frame_anchors", lib=L, handle=h, decode=0, conn=8, flags=0, lab=labels, lab_cap=npix * 4, tab=table, rows=64, count=n, mode=0,
             factor=1.0, scaled=None, d2=dist2, d2_cap=npix * 4, anch=anchors, klass=None, plane_cap=0):
        args = [handle, p(frame), 64, 48, factor, mode, decode, conn, 0, flags, p(klass), None, plane_cap, p(lab), lab_cap, p(tab), rows,
                C.addressof(count) if count is not None else None, p(scaled), C.byref(ow), C.byref(oh)]
        return getattr(lib, fn)(*(args + ([p(d2), d2_cap, p(anch)] if fn == "infur_frame_anchors" else [])))

    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48)
    r = FramePath(ctx).advance_regions(frame, 1.0, RAW, table_rows=64)
    assert n.value == r.n and (labels == r.labels).all() and (dist2 == reference(r.labels, SKIP, NONE, 64)[0]).all()
    assert (anchors == reference(r.labels, SKIP, NONE, 64)[1]).all()
    # every check and error of infur_frame_regions, call for call
    klass = np.zeros((48, 64), np.uint8)
    for kw in (dict(decode=2), dict(mode=2), dict(conn=5), dict(flags=2), dict(lab_cap=npix * 4 - 1), dict(factor=-1.0), dict(klass=klass, plane_cap=npix - 1),
               dict(klass=klass, plane_cap=npix), dict(tab=None, rows=0), dict(lab=None, lab_cap=0)):
        want = call(fn="infur_frame_regions", **kw)
        assert call(**kw) == want, kw
    assert call(lab_cap=npix * 4 - 1) == _lib.E_CAPACITY and call(conn=5) == _lib.E_INVALID_ARG and call(factor=-1.0) == _lib.E_INVALID_SCALE
    assert call(d2_cap=npix * 4 - 1) == _lib.E_CAPACITY and "distance plane" in ctx.last_error()
    assert call(d2=None, d2_cap=0) == _lib.OK  # no distances wanted: their capacity does not matter
    assert call(lab=None, tab=None, count=None, d2=None, anch=None) == _lib.E_INVALID_ARG  # nothing wanted
    assert call(lab=None, tab=None, count=None, d2=None, rows=0) == _lib.E_INVALID_ARG  # anchors without rows: not wanted
    assert call(lab=None, tab=None, count=None, d2=None) == _lib.OK and call(lab=None, tab=None, count=None, anch=None) == _lib.OK
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        a = FramePath(c).advance_anchors(frame, 0.5, RAW, want_scaled=True)
        assert a.labels is None and a.table is None and a.n is None and a.dist2 is None and a.anchors is None and a.scaled.shape == (24, 32, 3)
        assert (a.scaled == FramePath(c).advance_regions(frame, 0.5, RAW, want_scaled=True).scaled).all()
        dist2[:], anchors[:], n.value = 9, 9, 77
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED == call(fn="infur_frame_regions", lib=c.L, handle=c.h)
        assert (scaled == FramePath(c).advance_regions(frame, 1.0, RAW, want_scaled=True).scaled).all()
        assert (dist2 == 9).all() and (anchors == 9).all() and n.value == 77
        # a distance plane that is too short changes nothing about that: capacities are checked once a model is loaded
        assert call(lib=c.L, handle=c.h, d2_cap=3) == _lib.E_MODEL_NOT_LOADED


def test_anchors_calls_leave_the_existing_legs_and_the_cached_graphs_alone(blob50):
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
        before = [fg.advance_regions(fr, 1.0, SOFTMAX) for fr in frames]  # the existing leg, before any Anchors call on this context
        for it in range(8):
            fr = frames[it % 4]
            args = (fr, 1.0, SOFTMAX if it & 1 else RAW, 4 if it & 2 else 8)
            s = fg.advance_anchors(*args, want_klass=bool(it & 4), want_conf=bool(it & 4), want_labels=bool(it & 1))
            e = fe.advance_anchors(*args)
            assert s.n == e.n and (s.dist2 == e.dist2).all() and (s.anchors == e.anchors).all() and (s.table == e.table).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "an anchors call caused a capture"
        assert cached1 >= cached0, "an anchors call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the anchors calls were not replayed"
        for fr, b4 in zip(frames, before):  # and after: the same bytes
            now = fg.advance_regions(fr, 1.0, SOFTMAX)
            assert now.n == b4.n and all(getattr(now, f).tobytes() == getattr(b4, f).tobytes() for f in ("klass", "conf", "labels", "table"))


def test_composition_with_tracks_on_the_device(ctx, model):
    """infur_frame_tracks_dev, then infur_anchors_dev on the label plane it left on the device: an anchor per track, no dense
    plane to the host"""
    L, h = ctx.L, ctx.h
    hh, ww, rows = FRAME_H, FRAME_W, 512
    frames = [W.synth_frame(hh, ww, index=i) for i in (2, 3)]
    trk = C.c_void_p()
    ctx.check(L.infur_tracker_create(h, 0, 0, C.byref(trk)))
    d = Dev(ctx, bgr=frames[0].nbytes, labels=hh * ww * 4, table=rows * 80, n=4, tor=rows * 4, summary=16, anchors=rows * 8)
    try:
        P = d.ptr
        for frame in frames:
            d.poison("anchors")
            d.put("bgr", frame)
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            ctx.check(L.infur_frame_tracks_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 8, 2, _lib.REGIONS_SKIP_BACKGROUND, None, None, 0, P["labels"], hh * ww * 4,
                                               P["table"], rows, P["n"], None, C.byref(ow), C.byref(oh), trk, 1, P["tor"], None, None, P["summary"]))
            ctx.check(L.infur_anchors_dev(h, P["labels"], 4, hh, ww, SKIP, NONE, None, P["anchors"], rows))
            ctx.synchronize()
            n = int(d.get("n").view(np.uint32)[0])
            labels = d.get("labels").view(np.uint32).reshape(hh, ww)
            tor = d.get("tor").view(np.uint32)[:n]
            anchors = d.get("anchors").view(np.uint32).reshape(rows, 2)
            assert 1 < n <= rows and (anchors == reference(labels, SKIP, NONE, rows)[1]).all()
            by_track = {int(t): anchors[i].tolist() for i, t in enumerate(tor)}  # rows mapped through track_of_region
            assert len(by_track) == n and NONE not in by_track
            assert all(labels.ravel()[at] == np.flatnonzero(tor == t)[0] and d2 >= 1 for t, (at, d2) in by_track.items())
    finally:
        d.free()
        L.infur_tracker_destroy(trk)


# --------------------------------------------------------------------------- #
# 4. the command line
# --------------------------------------------------------------------------- #
def test_cli_round_trip(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip)]
    r = subprocess.run(base + ["--regions", "--min-pixels", "3", "--skip-background", "--max-regions", "4096", "--anchors", "--regions-out",
                               str(tmp_path / "labels.u32"), "--dist-out", str(tmp_path / "dist.u32")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    dist = np.frombuffer((tmp_path / "dist.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    for i, rec in enumerate(lines):
        rd, ra = reference(labels[i], SKIP, NONE, rec["n_regions"])
        assert (dist[i] == rd).all() and len(rec["regions"]) == rec["n_regions"] > 1
        for reg, (at, d2) in zip(rec["regions"], ra.tolist()):
            assert reg["anchor"] == [at % 128, at // 128] and reg["radius"] == round(float(np.sqrt(d2)), 2)
