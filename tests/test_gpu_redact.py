"""Redact on the GPU against tests/redact_ref.py: exact integers, so every comparison is ``==`` on whole arrays, on poisoned device
buffers with guard bytes behind them (``Dev`` of tests/test_gpu_anchors.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Redact, RedactCmd, RedactOut

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_ref as D  # noqa: E402
import regions_ref as R  # noqa: E402
from test_gpu_anchors import POISON, Dev, _hip  # noqa: E402

pytestmark = pytest.mark.gpu

# the wave tile, the 256-column step and its carry; the 64-row band and its last partial band; the longest sides
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (63, 3), (64, 5), (65, 70), (129, 66), (135, 241), (2, 16500), (1, 32768), (32768, 1))
CASES = ([(D.FILL, 0, 0)] + [(D.PIXELATE, b, 0) for b in (2, 5, 64, 256)] + [(D.BLUR, r, p) for r in (1, 3, 255) for p in (1, 3)])
COLOUR = 0x0A6432  # B 0x32, G 0x64, R 0x0A


def dev_redact(ctx, frame, plane, select, invert, mode, size, passes, colour=COLOUR, want=("out", "counts"), in_place=False, d=None):
    """infur_redact_dev on poisoned, guarded buffers -> (out, counts), None where not wanted (checked untouched); in_place: out is the frame"""
    h, w = plane.shape
    select = np.asarray(select, np.uint8)
    own = d is None
    d = d or Dev(ctx, frame=frame.nbytes, plane=plane.nbytes, select=select.size, out=frame.nbytes, counts=32)
    try:
        d.poison("out", "counts")
        for name, a in (("frame", frame), ("plane", plane), ("select", select)):
            d.put(name, a)
        out = None if "out" not in want else d.ptr["frame"] if in_place else d.ptr["out"]
        ctx.check(ctx.L.infur_redact_dev(ctx.h, d.ptr["frame"], d.ptr["plane"], plane.dtype.itemsize, h, w, d.ptr["select"] if select.size else None,
                                         select.size, int(invert), mode, size, passes, colour, out, d.ptr["counts"] if "counts" in want else None))
        ctx.synchronize()
        assert d.get("plane").tobytes() == plane.tobytes() and d.get("select").tobytes() == select.tobytes()  # the inputs are inputs
        got_out, got_counts = d.get("frame" if in_place else "out").reshape(h, w, 3), d.get("counts").view(np.uint32)
        assert in_place or d.get("frame").tobytes() == frame.tobytes()
        assert "out" in want or in_place or (got_out == POISON).all(), "out was not wanted and was written"
        assert "counts" in want or (got_counts.view(np.uint8) == POISON).all(), "counts were not wanted and were written"
        return got_out if "out" in want else None, got_counts if "counts" in want else None
    finally:
        if own:
            d.free()


def planes(h, w, elem_bytes):
    """(name, plane, select, invert); the u32 planes are label planes with INFUR_REGION_NONE pixels and fewer table rows than labels"""
    for name, klass in (("smooth", R.smooth(h, w, seed=h + w)), ("noise", R.noise(h, w, 3, seed=w))):
        if elem_bytes == 1:
            plane, rows = klass, int(klass.max())  # (the largest class lies beyond the table, unless the plane holds one class)
            mid = int(klass[h // 2, w // 2])
            select = np.arange(max(rows, 1)) == (mid if mid < rows else int(klass.min()))
        else:
            plane, _, n = R.label(klass, None, 8, min_pixels=2 if name == "noise" else 0, flags=1)
            select = np.arange(max(n - 1, 1)) % 3 == 0
        yield name, plane, select, False
        yield name + ", inverted", plane, select, True
    yield "nothing", plane, np.zeros(select.size, np.uint8), False
    yield "everything", plane, np.zeros(select.size, np.uint8), True


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_frames_equal_the_rule(ctx, elem_bytes, shape):
    assert ctx.L.infur_features() & _lib.FEATURE_REDACT  # (fails on a library without the feature)
    (h, w), frame = shape, np.random.default_rng(sum(shape)).integers(0, 256, shape + (3,), dtype=np.uint8)
    for name, plane, select, invert in planes(h, w, elem_bytes):
        d = Dev(ctx, frame=frame.nbytes, plane=plane.nbytes, select=select.size, out=frame.nbytes, counts=32)
        try:
            for mode, size, passes in CASES:
                ref_out, ref_counts = D.redact(frame, plane, select, mode, size, passes, COLOUR, invert)
                out, counts = dev_redact(ctx, frame, plane, select, invert, mode, size, passes, d=d)
                assert (counts == ref_counts).all(), (name, mode, size, passes, counts, ref_counts)
                assert (out == ref_out).all(), (name, mode, size, passes)
                assert name != "nothing" or (counts[D.C_STATUS] == D.NOTHING and (out == frame).all())
            assert ref_counts[D.C_OUTSIDE] or h * w < 64  # values beyond the table were there to be counted
        finally:
            d.free()


@pytest.mark.parametrize("side,ok", [(4096, True), (4097, False)])
def test_the_cap_of_the_averaging_modes(ctx, side, ok):
    (h, w), frame, plane = (4096, side), np.full((4096, side, 3), 255, np.uint8), np.zeros((4096, side), np.uint8)
    d = Dev(ctx, frame=frame.nbytes, plane=plane.nbytes, select=1, out=frame.nbytes, counts=32)
    try:
        for mode, size in ((D.BLUR, 1), (D.PIXELATE, 256), (D.FILL, 0)):
            if ok or mode == D.FILL:
                out, counts = dev_redact(ctx, frame, plane, [1], False, mode, size, 1, colour=0xFFFFFF, d=d)
                assert (out == 255).all() and counts[D.C_SELECTED] == h * w
            else:
                rc = ctx.L.infur_redact_dev(ctx.h, d.ptr["frame"], d.ptr["plane"], 1, h, w, d.ptr["select"], 1, 0, mode, size, 1, 0, d.ptr["out"], None)
                assert rc == _lib.E_INVALID_ARG and "2^24 pixels" in ctx.last_error()
    finally:
        d.free()


def some(h=65, w=70, elem_bytes=1, seed=3):
    klass = R.smooth(h, w, seed=seed)
    frame = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    plane = klass if elem_bytes == 1 else np.where(klass == klass[0, 0], 0xFFFFFFFF, klass).astype(np.uint32)
    return frame, plane, np.arange(21) % 2 == 0


@pytest.mark.parametrize("case", CASES, ids=str)
def test_in_place_and_each_output_alone(ctx, case):
    frame, plane, select = some()
    both = dev_redact(ctx, frame, plane, select, False, *case)
    assert (both[0] == D.redact(frame, plane, select, *case, COLOUR)[0]).all()
    there = dev_redact(ctx, frame, plane, select, False, *case, in_place=True)
    assert there[0].tobytes() == both[0].tobytes() and there[1].tobytes() == both[1].tobytes()
    assert dev_redact(ctx, frame, plane, select, False, *case, want=("out",))[0].tobytes() == both[0].tobytes()
    assert dev_redact(ctx, frame, plane, select, False, *case, want=("counts",))[1].tobytes() == both[1].tobytes()


def test_a_call_after_a_larger_frame_and_a_repeat(ctx):
    frame, plane, select = some(63, 3, seed=9)
    first = dev_redact(ctx, frame, plane, select, True, D.BLUR, 2, 3)
    big = some(129, 66, elem_bytes=4)
    assert (dev_redact(ctx, *big, True, D.BLUR, 4, 2)[0] == D.redact(*big, D.BLUR, 4, 2, invert=True)[0]).all()  # the scratch grows and is reused
    again = dev_redact(ctx, frame, plane, select, True, D.BLUR, 2, 3)
    assert first[0].tobytes() == again[0].tobytes() == D.redact(frame, plane, select, D.BLUR, 2, 3, invert=True)[0].tobytes()
    assert first[1].tobytes() == again[1].tobytes()


def test_the_device_call_inside_a_captured_graph(ctx):
    """launches only: a graph of the call replays to the eager bytes on whatever frame lies in the input buffer, replay after replay"""
    hip = _hip()
    h, w = 65, 70
    (f1, plane, select), (f2, _, _) = some(h, w, seed=3), some(h, w, seed=5)
    d = Dev(ctx, frame=f1.nbytes, plane=plane.nbytes, select=select.size, out=f1.nbytes, counts=32)
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    try:
        P, stream = d.ptr, C.c_void_p(ctx.stream)
        call = lambda: ctx.L.infur_redact_dev(ctx.h, P["frame"], P["plane"], 1, h, w, P["select"], select.size, 0, D.BLUR, 3, 3, 0, P["out"], P["counts"])  # noqa: E731
        for name, a in (("frame", f1), ("plane", plane), ("select", select.astype(np.uint8))):
            d.put(name, a)
        ctx.check(call())  # the warm call
        ctx.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for frame in (f2, f1, f2):
            d.poison("out", "counts")
            d.put("frame", frame)
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            replay = d.get("out"), d.get("counts")
            eager = dev_redact(ctx, frame, plane, select, False, D.BLUR, 3, 3, colour=0)
            ref = D.redact(frame, plane, select, D.BLUR, 3, 3)
            assert replay[0].tobytes() == eager[0].tobytes() == ref[0].tobytes() and replay[1].tobytes() == eager[1].tobytes() == ref[1].tobytes()
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_host_pointer_call_and_processor(ctx, elem_bytes):
    frame, plane, select = some(elem_bytes=elem_bytes)
    for mode, size, passes in ((D.FILL, 0, 0), (D.PIXELATE, 5, 0), (D.BLUR, 3, 2)):
        dev = dev_redact(ctx, frame, plane, select, True, mode, size, passes)
        out, counts, sel = np.empty_like(frame), np.zeros(8, np.uint32), np.ascontiguousarray(select, np.uint8)
        ctx.check(ctx.L.infur_redact(ctx.h, frame.ctypes.data, plane.ctypes.data, elem_bytes, *plane.shape, sel.ctypes.data, sel.size, 1, mode, size, passes,
                                     COLOUR, out.ctypes.data, counts.ctypes.data))
        assert out.tobytes() == dev[0].tobytes() and counts.tobytes() == dev[1].tobytes()
    proc, res = Redact(ctx), RedactOut()
    proc.control(RedactCmd.Blur(sel, 3, 2, invert=True)).advance((frame, plane), res)
    assert not proc.is_dirty() and res.out.tobytes() == out.tobytes() and res.counts.tobytes() == counts.tobytes() and not res.nothing


def test_rejected_calls_leave_the_buffers_untouched(ctx):
    L, (frame, plane, select) = ctx.L, some(6, 7)
    d = Dev(ctx, frame=frame.nbytes, plane=plane.nbytes, select=21, out=frame.nbytes, counts=32)
    try:
        P = d.ptr
        call = lambda fr=P["frame"], pl=P["plane"], elem=1, hh=6, ww=7, sel=P["select"], rows=21, flags=0, mode=D.BLUR, size=2, passes=1, out=P["out"], counts=P["counts"]: (  # noqa: E731
            L.infur_redact_dev(ctx.h, fr, pl, elem, hh, ww, sel, rows, flags, mode, size, passes, 0, out, counts))
        for kw, message in ((dict(elem=2), "elem_bytes"), (dict(flags=2), "unknown redact flags"), (dict(mode=3), "unknown redact mode"),
                            (dict(mode=D.PIXELATE, size=1), "2 to 256"), (dict(mode=D.PIXELATE, size=257), "2 to 256"), (dict(size=0), "1 to 255"),
                            (dict(size=256), "1 to 255"), (dict(passes=0), "passes"), (dict(passes=4), "passes"), (dict(hh=0), "1 to 32768"),
                            (dict(ww=32769), "1 to 32768"), (dict(hh=32768, ww=513), "2^24 pixels"), (dict(sel=None), "no select pointer"),
                            (dict(out=None, counts=None), "no output wanted"), (dict(pl=None), "no plane pointer"), (dict(fr=None), "no frame pointer"),
                            (dict(out=C.c_void_p(P["frame"].value + 3)), "overlaps the frame"),
                            (dict(elem=2, flags=2, mode=3, hh=0, sel=None), "elem_bytes"), (dict(flags=2, mode=3, hh=0, sel=None), "flags"),
                            (dict(mode=3, hh=0, sel=None), "mode"), (dict(size=0, hh=0, sel=None), "1 to 255"), (dict(hh=0, sel=None, out=None, counts=None), "1 to 32768"),
                            (dict(sel=None, out=None, counts=None, pl=None), "no select pointer"), (dict(out=None, counts=None, pl=None), "no output wanted")):
            assert call(**kw) == _lib.E_INVALID_ARG and message in ctx.last_error(), (kw, ctx.last_error())
        for name, a in (("frame", frame), ("plane", plane), ("select", select.astype(np.uint8))):
            d.put(name, a)
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("out", "counts"))
        assert call(mode=D.FILL, size=999, passes=9) == call(mode=D.PIXELATE, size=2, passes=9) == call(sel=None, rows=0, flags=1) == _lib.OK  # the next valid calls
        ctx.synchronize()
        assert (d.get("out").reshape(6, 7, 3) == D.redact(frame, plane, [], D.BLUR, 2, 1, invert=True)[0]).all()
    finally:
        d.free()


@pytest.mark.parametrize("h,w,factor", [(48, 64, 1.0), (48, 64, 0.5), (61, 97, 1.0)])
def test_frame_calls_equal_segments_then_redact(ctx, model, h, w, factor):
    L, fp = ctx.L, FramePath(ctx)
    frame = W.synth_frame(h, w, index=5)
    seg = fp.advance_segments(frame, factor, _lib.DECODE_RAW, want_scaled=True)
    oh_, ow_ = seg.klass.shape
    npix = oh_ * ow_
    cmd = RedactCmd.Blur([int(seg.klass[0, 0]), int(seg.klass[-1, -1])], 2, 2)
    table = cmd.table()
    d = Dev(ctx, bgr=frame.nbytes, select=table.size, klass=npix, scaled=npix * 3, redacted=npix * 3, counts=32, klass2=npix, conf=npix, scaled2=npix * 3)
    try:
        P, ow, oh = d.ptr, C.c_uint32(0), C.c_uint32(0)
        d.put("bgr", frame)
        d.put("select", table)
        ctx.check(L.infur_frame_segments_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, P["klass"], None, npix, None, 0, None, 0, P["scaled"],
                                             C.byref(ow), C.byref(oh)))
        ctx.check(L.infur_redact_dev(ctx.h, P["scaled"], P["klass"], 1, oh.value, ow.value, P["select"], table.size, 0, cmd.mode, cmd.size, cmd.passes, 0,
                                     P["redacted"], P["counts"]))
        ctx.synchronize()
        chain = d.get("redacted"), d.get("counts")
        assert (ow.value, oh.value) == (ow_, oh_) and d.get("klass").tobytes() == seg.klass.tobytes() and d.get("scaled").tobytes() == seg.scaled.tobytes()
        assert chain[0].tobytes() == D.redact(seg.scaled, seg.klass, table, cmd.mode, cmd.size, cmd.passes)[0].tobytes()
        for scaled in (P["scaled2"], None):  # with and without the caller's scaled frame (None at 1.0: the frame itself is read)
            d.poison("redacted", "counts", "klass2", "conf")
            ctx.check(L.infur_frame_redact_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, P["select"], table.size, 0, cmd.mode, cmd.size, cmd.passes,
                                               0, P["redacted"], npix * 3, P["klass2"] if scaled else None, P["conf"] if scaled else None, npix,
                                               P["counts"], scaled, C.byref(ow), C.byref(oh)))
            ctx.synchronize()
            assert d.get("redacted").tobytes() == chain[0].tobytes() and d.get("counts").tobytes() == chain[1].tobytes()
            if scaled:
                assert d.get("klass2").tobytes() == seg.klass.tobytes() and d.get("conf").tobytes() == seg.conf.tobytes()
                assert d.get("scaled2").tobytes() == seg.scaled.tobytes()
        assert L.infur_frame_redact_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, P["select"], table.size, 0, cmd.mode, cmd.size, cmd.passes, 0,
                                        P["redacted"], npix * 3 - 1, None, None, 0, None, None, C.byref(ow), C.byref(oh)) == _lib.E_CAPACITY
    finally:
        d.free()
    r = fp.advance_redact(frame, cmd, factor, want_klass=True, want_conf=True, want_scaled=True)  # infur_frame_redact, host pointers
    assert r.redacted.tobytes() == chain[0].tobytes() and r.counts.tobytes() == chain[1].tobytes()
    assert (r.klass == seg.klass).all() and (r.conf == seg.conf).all() and (r.scaled == seg.scaled).all()


def test_frame_calls_without_a_model():
    frame = W.synth_frame(48, 64, index=5)
    with Context(device=0) as c:
        want = FramePath(c).advance_segments(frame, 0.5, _lib.DECODE_RAW, want_scaled=True).scaled
        r = FramePath(c).advance_redact(frame, RedactCmd.Fill([0]), 0.5, want_scaled=True)  # infur_frame_redact
        assert r.redacted is None and r.counts is None and (r.scaled == want).all()
        d, ow, oh = Dev(c, bgr=frame.nbytes, select=1, redacted=want.nbytes, scaled=want.nbytes), C.c_uint32(0), C.c_uint32(0)
        try:
            d.put("bgr", frame)
            for cap in (want.nbytes, 3):  # capacities are checked once a model is loaded
                d.poison("scaled")
                assert c.L.infur_frame_redact_dev(c.h, d.ptr["bgr"], 64, 48, 0.5, 0, 0, d.ptr["select"], 1, 0, D.FILL, 0, 0, 0, d.ptr["redacted"], cap, None,
                                                  None, 0, None, d.ptr["scaled"], C.byref(ow), C.byref(oh)) == _lib.E_MODEL_NOT_LOADED
                c.synchronize()
                assert d.get("scaled").tobytes() == want.tobytes() and (d.get("redacted") == POISON).all()
        finally:
            d.free()
