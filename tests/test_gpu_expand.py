"""Expand on the GPU: every output of ``infur_expand*`` and of the fused ``infur_frame_expand*`` against the brute force of
tests/expand_ref.py.  Everything is an integer, exact and a function of the plane alone, so every comparison is ``==`` on whole
arrays, on poisoned device buffers with guard bytes behind them (``Dev`` of tests/test_gpu_anchors.py)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Expand, ExpandCmd, ExpandOut, FramePath, expand_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_ref as E  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402
from test_gpu_anchors import POISON, Dev, _hip  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
OUTPUTS = ("out", "dist2", "source", "table", "counts")
# (63,3) (64,5) (65,70) (129,66): the coarse step of 64 rows and its last partial block; (2,16500) (1,32768) (32768,1): the tile
# carry of the row pass and the longest sides
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (63, 3), (64, 5), (65, 70), (129, 66), (135, 241), (2, 16500), (1, 32768), (32768, 1))


def dev_expand(ctx, plane, open_value, reach=0, rows=22, want=OUTPUTS):
    """infur_expand_dev on poisoned, guarded device buffers -> the wanted outputs by name (the others are checked to be untouched)"""
    h, w = plane.shape
    d = Dev(ctx, plane=plane.nbytes, out=plane.nbytes, dist2=h * w * 4, source=h * w * 4, table=rows * 16, counts=32)
    try:
        d.put("plane", plane)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_expand_dev(ctx.h, d.ptr["plane"], plane.dtype.itemsize, h, w, 0, open_value, reach, p("out"), p("dist2"), p("source"),
                                         p("table"), rows, p("counts")))
        ctx.synchronize()
        assert d.get("plane").tobytes() == plane.tobytes()  # the input is an input
        got = {"out": d.get("out").view(plane.dtype).reshape(h, w), "dist2": d.get("dist2").view(np.uint32).reshape(h, w),
               "source": d.get("source").view(np.uint32).reshape(h, w), "table": d.get("table").view(np.uint32).reshape(rows, 4),
               "counts": d.get("counts").view(np.uint32)}
        for name in OUTPUTS:
            if name not in want:
                assert (got.pop(name).view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return got
    finally:
        d.free()


@functools.lru_cache(maxsize=None)
def _near(shape, mask_bytes):
    return E.nearest(np.frombuffer(mask_bytes, bool).reshape(shape))


def reference(plane, open_value, reach=0, rows=22):
    """the brute force's answer by output name; the nearest seeds are computed once per set of open pixels and left unchanged"""
    is_open = plane == plane.dtype.type(open_value)
    return dict(zip(OUTPUTS, E.expand(plane, open_value, reach, rows, near=_near(plane.shape, is_open.tobytes()))))


def check(ctx, plane, open_value, reach=0, rows=22, want=OUTPUTS, name=""):
    ref, got = reference(plane, open_value, reach, rows), dev_expand(ctx, plane, open_value, reach, rows, want)
    for key in want:
        assert (got[key] == ref[key]).all(), (name, plane.shape, plane.dtype, open_value, reach, key)
    return ref


def planes(h, w):
    """(name, class plane, the class to open): regions_ref's families with one value opened, then the edge planes"""
    # (the brute force pairs every open pixel with every seed: the largest shape takes three families, the long ones the sparse planes)
    for name, make in (("smooth", lambda: R.smooth(h, w, seed=h + w)), ("noise3", lambda: R.noise(h, w, 3, seed=w)), ("noise21", lambda: R.noise(h, w, 21, seed=h)),
                       ("vstripes", lambda: R.stripes(h, w, vertical=True)), ("hstripes", lambda: R.stripes(h, w, vertical=False)),
                       ("staircase", lambda: R.staircase(h, w)))[:0 if h * w > 135 * 241 else 3 if h * w > 10000 else 6]:
        k = make()
        yield name, k, int(k[h // 2, w // 2])
    yield "checkerboard", R.checkerboard(h, w), 0
    sparse = R.noise(h, w, 200, seed=h * w)
    yield "few seeds", np.where(sparse < 3, sparse + 1, 0).astype(np.uint8), 0
    yield "few open", np.where(sparse < 3, 0, sparse).astype(np.uint8), 0
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        k = np.zeros((h, w), np.uint8)
        k[y, x] = 3
        yield f"corner {y},{x}", k, 0
    row, col = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    row[h // 2], col[:, w // 3] = 2, 3
    yield "seed row", row, 0
    yield "seed column", col, 0
    yield "no seed", R.single(h, w), 3
    yield "all seeds", R.single(h, w), 0


def as_elem(klass, open_class, elem_bytes):
    return (klass, open_class) if elem_bytes == 1 else (U.as_u32(klass), int(U.u32_table()[open_class]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_planes_equal_the_brute_force(ctx, elem_bytes, shape):
    assert ctx.L.infur_features() & _lib.FEATURE_EXPAND  # (fails on a library without the feature)
    for name, klass, open_class in planes(*shape):
        plane, open_value = as_elem(klass, open_class, elem_bytes)
        ref = check(ctx, plane, open_value, name=name)
        d2 = ref["dist2"][plane == open_value].astype(np.int64)
        exact = [r for r in range(2, 200) if (d2 == r * r).any()][-1:]  # a reach whose square is a distance the plane holds
        for reach in [1, 5] + exact:
            got = check(ctx, plane, open_value, reach, name=name)
            assert not exact or reach != exact[0] or (got["out"][ref["dist2"] == reach * reach] != open_value).all()
        if name == "no seed":
            assert ref["counts"][E.C_STATUS] == E.NO_SEED and (ref["dist2"] == NONE).all() and (ref["source"] == NONE).all()
        if name == "corner 0,0" and shape == (135, 241):
            assert exact == [199] and ref["counts"][E.C_MAX_D2] == 134 * 134 + 240 * 240  # every distance long


def test_rows_below_equal_and_above_the_number_of_values(ctx):
    labels, _, n = R.label(R.smooth(65, 70), None, 8, min_pixels=20, flags=1)
    assert n > 4 and (labels == NONE).any()
    for rows in (1, n - 1, n, n + 9):
        ref = check(ctx, labels, NONE, reach=3, rows=rows)
        assert (ref["table"][:n, E.SEEDS] > 0).all() and (ref["table"][n:] == [0, 0, 0, NONE]).all()  # every row is written


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_each_output_alone(ctx, elem_bytes):
    for klass in (R.smooth(65, 70), R.noise(7, 65, 3), R.noise(1, 5, 3)):
        plane, open_value = as_elem(klass, int(klass[0, 0]), elem_bytes)
        for name in OUTPUTS:
            check(ctx, plane, open_value, reach=2, rows=9, want=(name,))
        check(ctx, plane, open_value, reach=2, rows=0, want=("out", "dist2", "source", "counts"))  # a table pointer with no rows is no table


def test_a_call_after_a_larger_plane_and_a_repeat(ctx):
    k = R.noise(63, 3, 3, seed=9)
    first = dev_expand(ctx, k, 0, 2)
    check(ctx, R.smooth(129, 66), 1)  # a larger plane in between: the scratch grows and is reused
    again = dev_expand(ctx, k, 0, 2)
    assert all(first[key].tobytes() == again[key].tobytes() for key in OUTPUTS)
    check(ctx, k, 0, 2)


def test_the_device_call_inside_a_captured_graph(ctx):
    """after one call outside the capture the scratch is there: the call is launches only, and a graph of them replays to the eager
    bytes on whatever plane lies in the input buffer, replay after replay"""
    hip = _hip()
    h, w, rows = 65, 70, 9
    first, second = R.smooth(h, w, seed=3), R.noise(h, w, 3, seed=5)
    d = Dev(ctx, plane=h * w, out=h * w, dist2=h * w * 4, source=h * w * 4, table=rows * 16, counts=32)
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    try:
        P, stream = d.ptr, C.c_void_p(ctx.stream)
        call = lambda: ctx.L.infur_expand_dev(ctx.h, P["plane"], 1, h, w, 0, 0, 4, P["out"], P["dist2"], P["source"], P["table"], rows, P["counts"])  # noqa: E731
        d.put("plane", first)
        ctx.check(call())  # the warm call
        ctx.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for plane in (second, first, second):
            d.poison(*OUTPUTS)
            d.put("plane", plane)
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            eager = dev_expand(ctx, plane, 0, 4, rows)
            for key in OUTPUTS:
                assert d.get(key).tobytes() == eager[key].tobytes() == reference(plane, 0, 4, rows)[key].tobytes(), key
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


def test_rejected_calls_leave_the_buffers_untouched(ctx):
    L, h = ctx.L, ctx.h
    d = Dev(ctx, plane=42 * 4, out=42 * 4, dist2=42 * 4, source=42 * 4, table=16 * 5, counts=32)
    try:
        d.put("plane", U.as_u32(R.noise(6, 7, 3)))
        P = d.ptr
        call = lambda elem=4, flags=0, opn=0, hh=6, ww=7, pl=P["plane"], out=P["out"], dist2=P["dist2"], source=P["source"], table=P["table"], rows=5, counts=P["counts"]: (  # noqa: E731
            L.infur_expand_dev(h, pl, elem, hh, ww, flags, opn, 2, out, dist2, source, table, rows, counts))
        nothing = dict(out=None, dist2=None, source=None, table=None, counts=None)
        for kw, message in ((dict(elem=2), "elem_bytes"), (dict(flags=1), "unknown expand flags"), (dict(elem=1, opn=256), "open_value"),
                            (dict(hh=32769), "up to 32768"), (dict(ww=32769), "up to 32768"), (nothing, "no output wanted"),
                            (dict(out=None, dist2=None, source=None, counts=None, rows=0), "no output wanted"), (dict(pl=None), "no plane pointer"),
                            (dict(out=P["plane"]), "in place"),
                            # the order of the checks: element size, flag bits, open value, sides, nothing wanted, pointers
                            (dict(elem=2, flags=1, hh=32769, pl=None, **nothing), "elem_bytes"), (dict(elem=1, flags=1, opn=256, hh=32769, **nothing), "flags"),
                            (dict(elem=1, opn=256, hh=32769, **nothing), "open_value"), (dict(hh=32769, pl=None, **nothing), "up to 32768"),
                            (dict(pl=None, **nothing), "no output wanted")):
            assert call(**kw) == _lib.E_INVALID_ARG and message in ctx.last_error(), kw
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in OUTPUTS)
        for hh, ww in ((0, 7), (6, 0)):  # an empty plane: zero rows, zero counts and nothing else
            assert call(hh=hh, ww=ww, pl=None) == _lib.OK
            ctx.synchronize()
            assert d.get("table").view(np.uint32).reshape(5, 4).tolist() == [[0, 0, 0, NONE]] * 5 and not d.get("counts").any()
            assert all((d.get(name) == POISON).all() for name in ("out", "dist2", "source"))
        assert call(hh=32768, ww=1, pl=None) == _lib.E_INVALID_ARG and "no plane pointer" in ctx.last_error()  # 32768 itself is a side
    finally:
        d.free()


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_host_pointer_call_and_processor(ctx, elem_bytes):
    proc = Expand(ctx)
    for klass in (R.smooth(65, 70), R.noise(7, 65, 3)):
        plane, open_value = as_elem(klass, int(klass[0, 0]), elem_bytes)
        out = ExpandOut(rows=22, want_source=True)
        proc.control(ExpandCmd.Grow(open_value, 3)).advance(plane, out)
        ref = reference(plane, open_value, 3)
        assert not proc.is_dirty() and all((getattr(out, key) == ref[key]).all() for key in OUTPUTS)
        recs = expand_summary(out.table)
        assert [r["value"] for r in recs] == np.flatnonzero(ref["table"][:, E.SEEDS]).tolist()
        assert all(r["margin"] == round(math.sqrt(int(ref["table"][r["value"], E.MAX_D2])), 2) <= 3 for r in recs)


def test_fused_path_equals_regions_then_the_brute_force(ctx, model):
    fp = FramePath(ctx)
    frame = W.synth_frame(96, 128, index=5)
    kw = dict(decode=_lib.DECODE_SOFTMAX, min_pixels=6, flags=_lib.REGIONS_SKIP_BACKGROUND, table_rows=4096)
    r = fp.advance_regions(frame, 1.0, **kw)
    assert r.n > 1 and (r.labels == NONE).any()
    for reach in (0, 4):
        e = fp.advance_expand(frame, reach, 1.0, want_source=True, **kw)
        ref = reference(r.labels, NONE, reach, r.n)
        assert e.n == r.n and (e.labels == r.labels).all() and (e.table == r.table).all() and (e.klass == r.klass).all() and (e.conf == r.conf).all()
        for got, key in ((e.grown, "out"), (e.dist2, "dist2"), (e.source, "source"), (e.expand_table, "table"), (e.expand_counts, "counts")):
            assert (got == ref[key]).all(), (reach, key)
    q = fp.advance_expand(frame, 4, 1.0, want_labels=False, want_klass=False, want_conf=False, want_dist2=False, **kw)  # labels go to scratch
    assert q.labels is None and q.dist2 is None and (q.grown == ref["out"]).all() and (q.expand_table == ref["table"]).all()
    # every check and error before Expand is infur_frame_regions' own
    npix, n, ow, oh = 96 * 128, C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    buf = np.full((96, 128), 9, np.uint32)
    for conn, lab_cap, factor in ((5, npix * 4, 1.0), (8, npix * 4 - 1, 1.0), (8, npix * 4, -1.0)):
        args = [ctx.h, frame.ctypes.data, 128, 96, factor, 0, 0, conn, 0, 0, None, None, 0, buf.ctypes.data, lab_cap, None, 0, C.addressof(n), None,
                C.byref(ow), C.byref(oh)]
        want = ctx.L.infur_frame_regions(*args)
        assert want != _lib.OK and ctx.L.infur_frame_expand(*(args + [0, buf.ctypes.data, npix * 4, None, 0, None, 0, None, 0, None])) == want
    assert ctx.L.infur_frame_expand(*(args[:4] + [1.0] + args[5:] + [0, buf.ctypes.data, npix * 4 - 1, None, 0, None, 0, None, 0, None])) == _lib.E_CAPACITY
