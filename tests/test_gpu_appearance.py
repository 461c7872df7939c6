"""Appearance on the GPU against tests/appearance_ref.py: exact integers, so every comparison is ``==`` on whole arrays, on poisoned
device buffers with guard bytes behind them (``Dev`` of tests/test_gpu_anchors.py), for the _dev form and the host-pointer form."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Appearance, AppearanceCmd, AppearanceOut, Context, FramePath, appearance_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import appearance_ref as A  # noqa: E402
import regions_ref as R  # noqa: E402
from test_gpu_anchors import POISON, Dev, _hip  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TILE_ROWS, SLOTS = 32, 16  # appearance.hip: a workgroup's tile is 64 columns x 32 rows and keeps 16 values in LDS
NAMES = ("table", "hist", "counts")


def sizes(plane, rows):
    return dict(frame=plane.size * 3, plane=plane.nbytes, table=rows * 96, hist=rows * 256, counts=32)


def views(d):
    return d.get("table").view(np.uint64).reshape(-1, 12), d.get("hist").view(np.uint32).reshape(-1, 64), d.get("counts").view(np.uint32)


def dev_appearance(ctx, frame, plane, rows, flags=0, skip=0, want=NAMES, d=None, poison=True):
    """infur_appearance_dev on poisoned, guarded buffers -> (table, hist, counts), None where not wanted (checked untouched)"""
    own, d = d is None, d or Dev(ctx, **sizes(plane, rows))
    try:
        if poison:
            d.poison(*NAMES)
        d.put("frame", frame)
        d.put("plane", plane)
        ctx.check(ctx.L.infur_appearance_dev(ctx.h, d.ptr["frame"], d.ptr["plane"], plane.dtype.itemsize, *plane.shape, flags, skip,
                                             d.ptr["table"] if "table" in want else None, rows, d.ptr["hist"] if "hist" in want else None,
                                             d.ptr["counts"] if "counts" in want else None))
        ctx.synchronize()
        assert d.get("frame").tobytes() == frame.tobytes() and d.get("plane").tobytes() == plane.tobytes()  # the inputs are inputs
        got = views(d)
        assert all(name in want or (a.view(np.uint8) == POISON).all() for name, a in zip(NAMES, got)), "an unwanted output was written"
        return tuple(a if name in want else None for name, a in zip(NAMES, got))
    finally:
        if own:
            d.free()


def host_appearance(ctx, frame, plane, rows, flags=0, skip=0):
    out = np.full((rows, 12), POISON, np.uint64), np.full((rows, 64), POISON, np.uint32), np.full(8, POISON, np.uint32)
    ctx.check(ctx.L.infur_appearance(ctx.h, frame.ctypes.data, plane.ctypes.data, plane.dtype.itemsize, *plane.shape, flags, skip, out[0].ctypes.data,
                                     rows, out[1].ctypes.data, out[2].ctypes.data))
    return out


def check(ctx, frame, plane, rows, flags=0, skip=0, name=""):
    ref = A.appearance(frame, plane, rows, flags, skip)
    for form in (dev_appearance, host_appearance):
        for what, got, want in zip(NAMES, form(ctx, frame, plane, rows, flags, skip), ref):
            assert (got == want).all(), (name, form.__name__, what)
    return ref


def random_frame(h, w, seed=0):
    return np.random.default_rng(seed + h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)


# a pixel, the header's row, fewer columns than channels, one column, one row of several waves; w * 3 no multiple of 4; the wave's
# width and its neighbours; the tile's rows and their neighbours
SHAPES = ((1, 1), (1, 6), (5, 3), (70, 1), (1, 200), (61, 97), (9, 63), (9, 64), (9, 65), (9, 129), (TILE_ROWS - 1, 70), (TILE_ROWS, 70),
          (TILE_ROWS + 1, 70))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_planes_equal_the_rule(ctx, elem_bytes, shape):
    assert ctx.L.infur_features() & _lib.FEATURE_APPEARANCE  # (fails on a library without the feature)
    (h, w), frame = shape, random_frame(*shape)
    for name, klass in (("smooth", R.smooth(h, w, seed=h + w)), ("noise", R.noise(h, w, 3 * SLOTS, seed=w))):
        if elem_bytes == 1:
            plane, rows = klass, max(int(klass.max()), 1)  # (the largest class lies beyond the table, unless the plane holds one class)
            check(ctx, frame, plane, rows, name=name)
            check(ctx, frame, plane, rows, A.SKIP, int(klass[0, 0]), name=name + ", skip")
        else:  # a label plane with INFUR_REGION_NONE pixels and fewer rows than labels, with and without SKIP
            plane, _, n = R.label(klass, None, 8, min_pixels=2 if name == "noise" else 0, flags=1)
            check(ctx, frame, plane, max(n - 1, 1), A.SKIP, NONE, name=name)
            check(ctx, frame, plane, max(n - 1, 1), name=name + ", none counted")


def special(name):
    """-> (frame, plane, rows): the planes and pictures that stress one path each"""
    if name == "many workgroups":  # 270 x 480: 9 x 8 tiles flush into the same rows
        return random_frame(270, 480), R.smooth(270, 480, seed=1), 21
    if name == "a value per pixel":  # every run goes down the no-slot path once the tile's slots are taken
        return random_frame(61, 97), np.arange(61 * 97, dtype=np.uint32).reshape(61, 97), 61 * 97
    if name == "alternating":  # 64 runs per wave
        return random_frame(9, 129), (np.indices((9, 129)).sum(0) % 2).astype(np.uint8), 2
    if name == "boundary at lanes 63 | 0":
        return random_frame(35, 128), np.repeat(np.array([[1, 2]], np.uint32), 64, axis=1).repeat(35, axis=0), 3
    if name == "one row, the rest outside":
        return random_frame(40, 70), R.smooth(40, 70, seed=2), 1
    if name == "all 255":  # the largest packed and in-LDS sums: one value over more than one full tile
        return np.full((70, 130, 3), 255, np.uint8), np.full((70, 130), 3, np.uint8), 4
    if name == "all 255, many runs":  # the largest packed sums of the segmented scan: runs of 64 and of 1
        plane = np.full((70, 130), 3, np.uint8)
        plane[::2, 64] = 1
        return np.full((70, 130, 3), 255, np.uint8), plane, 4
    if name == "one flat colour":  # every lane in one bin
        return np.full((40, 70, 3), (200, 100, 30), np.uint8), R.smooth(40, 70, seed=3), 21
    if name == "channels that differ":  # BG, BR and GR are not symmetric by accident
        y, x = np.indices((40, 70))
        return np.stack([x * 3 % 256, 255 - y * 5 % 256, (x * y) % 251], axis=2).astype(np.uint8), R.smooth(40, 70, seed=4), 21
    raise KeyError(name)


SPECIAL = ("many workgroups", "a value per pixel", "alternating", "boundary at lanes 63 | 0", "one row, the rest outside", "all 255",
           "all 255, many runs", "one flat colour", "channels that differ")


@pytest.mark.parametrize("name", SPECIAL)
def test_the_paths_and_the_arithmetic(ctx, name):
    frame, plane, rows = special(name)
    table, _, counts = check(ctx, frame, plane, rows, name=name)
    assert name != "one row, the rest outside" or counts[A.C_OUTSIDE] > 0
    assert name != "all 255" or table[3].tolist() == [9100] + [9100 * 255] * 3 + [9100 * 65025] * 6 + [63, 9100]


def test_output_subsets_and_a_repeat(ctx):
    frame, plane, rows = random_frame(65, 70), R.smooth(65, 70, seed=5), 21
    d = Dev(ctx, **sizes(plane, rows))
    try:
        full = dev_appearance(ctx, frame, plane, rows, A.SKIP, 0, d=d)
        again = dev_appearance(ctx, frame, plane, rows, A.SKIP, 0, d=d, poison=False)  # on the first call's results: the clear launch
        for k, name in enumerate(NAMES):
            alone = dev_appearance(ctx, frame, plane, rows, A.SKIP, 0, want=(name,), d=d)
            assert alone[k].tobytes() == full[k].tobytes() == again[k].tobytes()
    finally:
        d.free()
    proc, res = Appearance(ctx, AppearanceCmd(rows, skip=0)), AppearanceOut()
    proc.advance((frame, plane), res)
    assert not proc.is_dirty() and not res.nothing and all(getattr(res, name).tobytes() == full[k].tobytes() for k, name in enumerate(NAMES))
    recs = appearance_summary(res.table, res.hist)
    assert [r["value"] for r in recs] == np.flatnonzero(full[0][:, 0]).tolist() and abs(sum(recs[0]["histogram"]) - 1) < 1e-9
    v = recs[0]["value"]
    assert np.allclose(recs[0]["mean"], frame[plane == v].mean(0), atol=0.006) and np.allclose(recs[0]["std"], frame[plane == v].std(0), atol=0.006)


def test_the_device_call_inside_a_captured_graph(ctx):
    """launches only: a graph of the call replays to the eager bytes on whatever frame lies in the input buffer, replay after replay"""
    hip, (h, w), rows = _hip(), (65, 70), 21
    plane, d = R.smooth(h, w, seed=5), None
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    try:
        d = Dev(ctx, **sizes(plane, rows))
        P, stream = d.ptr, C.c_void_p(ctx.stream)
        call = lambda: ctx.L.infur_appearance_dev(ctx.h, P["frame"], P["plane"], 1, h, w, 0, 0, P["table"], rows, None, P["counts"])  # noqa: E731
        dev_appearance(ctx, random_frame(h, w), plane, rows, want=("table", "counts"), d=d)  # the warm call: the scratch histogram
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for seed in (1, 2, 1):
            frame = random_frame(h, w, seed)
            d.poison("table", "counts")
            d.put("frame", frame)
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            ref = A.appearance(frame, plane, rows)
            assert (views(d)[0] == ref[0]).all() and (views(d)[2] == ref[2]).all()
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        if d:
            d.free()


def test_rejected_calls_leave_the_buffers_untouched(ctx):
    frame, plane = random_frame(6, 7), R.noise(6, 7, 3, seed=1)
    d = Dev(ctx, **sizes(plane, 3))
    try:
        P = d.ptr
        call = lambda fr=P["frame"], pl=P["plane"], elem=1, hh=6, ww=7, flags=0, skip=0, table=P["table"], hist=P["hist"], counts=P["counts"]: (  # noqa: E731
            ctx.L.infur_appearance_dev(ctx.h, fr, pl, elem, hh, ww, flags, skip, table, 3, hist, counts))
        for kw, message in ((dict(elem=2), "elem_bytes"), (dict(flags=2), "unknown appearance flags"), (dict(hh=0), "1 to 32768"),
                            (dict(ww=32769), "1 to 32768"), (dict(table=None, hist=None, counts=None), "no output wanted"),
                            (dict(pl=None), "no plane pointer"), (dict(fr=None), "no frame pointer"), (dict(counts=P["frame"]), "overlaps the frame"),
                            (dict(elem=2, flags=2, hh=0, fr=None), "elem_bytes"), (dict(flags=2, hh=0, fr=None), "flags"),
                            (dict(hh=0, table=None, hist=None, counts=None, fr=None), "1 to 32768"),
                            (dict(table=None, hist=None, counts=None, fr=None), "no output wanted")):
            assert call(**kw) == _lib.E_INVALID_ARG and message in ctx.last_error(), (kw, ctx.last_error())
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in NAMES)
        d.put("frame", frame)
        d.put("plane", plane)
        assert call() == _lib.OK  # the next valid call
        ctx.synchronize()
        assert all((got == want).all() for got, want in zip(views(d), A.appearance(frame, plane, 3)))
    finally:
        d.free()


@pytest.mark.parametrize("h,w,factor", [(48, 64, 1.0), (48, 64, 0.5), (61, 97, 1.0)])
def test_frame_calls_equal_regions_then_appearance(ctx, model, h, w, factor):
    L, fp, rows = ctx.L, FramePath(ctx), 512
    frame = W.synth_frame(h, w, index=5)
    seg = fp.advance_segments(frame, factor, _lib.DECODE_RAW, want_scaled=True)
    npix = seg.klass.size
    reg = dict(klass=npix, conf=npix, labels=npix * 4, table=rows * 80, n=4, scaled=npix * 3)
    app = dict(atable=rows * 96, ahist=rows * 256, acounts=32)
    d = Dev(ctx, bgr=frame.nbytes, **reg, **app, **{k + "2": v for k, v in {**reg, **app}.items()})
    try:
        P, ow, oh = d.ptr, C.c_uint32(0), C.c_uint32(0)
        d.put("bgr", frame)
        front = lambda s: [ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, 8, 4, 1, P["klass" + s], P["conf" + s], npix, P["labels" + s], npix * 4,  # noqa: E731
                           P["table" + s], rows, P["n" + s], P["scaled" + s], C.byref(ow), C.byref(oh)]
        ctx.check(L.infur_frame_regions_dev(*front("")))
        ctx.check(L.infur_appearance_dev(ctx.h, P["scaled"], P["labels"], 4, oh.value, ow.value, A.SKIP, NONE, P["atable"], rows, P["ahist"], P["acounts"]))
        ctx.synchronize()
        n, scaled, labels = int(d.get("n").view(np.uint32)[0]), d.get("scaled").reshape(seg.scaled.shape), d.get("labels").view(np.uint32)
        ref = A.appearance(scaled, labels, rows, A.SKIP, NONE)
        assert 0 < n < rows and (scaled == seg.scaled).all() and all((got == want).all() for got, want in zip(
            (d.get("atable").view(np.uint64).reshape(-1, 12), d.get("ahist").view(np.uint32).reshape(-1, 64), d.get("acounts").view(np.uint32)), ref))
        assert not ref[0][n:].any() and ref[0][:n, 0].all()  # rows beyond the region count are zero
        ctx.check(L.infur_frame_appearance_dev(*front("2"), P["atable2"], rows, P["ahist2"], P["acounts2"]))
        ctx.synchronize()
        assert all(d.get(name + "2").tobytes() == d.get(name).tobytes() for name in list(reg) + list(app))
        d.poison("atable2", "ahist2", "acounts2", "labels2", "scaled2")  # nothing of Regions' wanted, no scaled frame (at 1.0 the frame itself is read)
        ctx.check(L.infur_frame_appearance_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, 8, 4, 1, None, None, 0, None, 0, None, 0, None, None,
                                               C.byref(ow), C.byref(oh), P["atable2"], rows, None, P["acounts2"]))
        ctx.synchronize()
        assert all(d.get(name + "2").tobytes() == d.get(name).tobytes() for name in ("atable", "acounts"))
        assert all((d.get(name) == POISON).all() for name in ("ahist2", "labels2", "scaled2"))
        chain = d.get("atable").view(np.uint64).reshape(-1, 12), d.get("ahist").view(np.uint32).reshape(-1, 64), d.get("acounts").view(np.uint32)
    finally:
        d.free()
    r = fp.advance_appearance(frame, factor, min_pixels=4, flags=1, table_rows=rows, want_scaled=True)  # infur_frame_appearance, host pointers
    assert r.n == n and (r.labels.ravel() == labels).all() and (r.scaled == seg.scaled).all() and (r.klass == seg.klass).all()
    assert (r.appearance_table == chain[0][:n]).all() and (r.appearance_hist == chain[1][:n]).all() and (r.appearance_counts == chain[2]).all()


def test_frame_calls_without_a_model():
    frame = W.synth_frame(48, 64, index=5)
    with Context(device=0) as c:
        want = FramePath(c).advance_segments(frame, 0.5, _lib.DECODE_RAW, want_scaled=True).scaled
        r = FramePath(c).advance_appearance(frame, 0.5, want_scaled=True)  # infur_frame_appearance
        assert r.appearance_table is None and r.appearance_counts is None and r.labels is None and (r.scaled == want).all()
        d, ow, oh = Dev(c, bgr=frame.nbytes, atable=96, ahist=256, acounts=32, labels=want.size // 3 * 4, scaled=want.nbytes), C.c_uint32(0), C.c_uint32(0)
        try:
            d.put("bgr", frame)
            assert c.L.infur_frame_appearance_dev(c.h, d.ptr["bgr"], 64, 48, 0.5, 0, 0, 8, 0, 0, None, None, 0, d.ptr["labels"], 3, None, 0, None,
                                                  d.ptr["scaled"], C.byref(ow), C.byref(oh), d.ptr["atable"], 1, d.ptr["ahist"],
                                                  d.ptr["acounts"]) == _lib.E_MODEL_NOT_LOADED  # (capacities are checked once a model is loaded)
            c.synchronize()
            assert d.get("scaled").tobytes() == want.tobytes() and all((d.get(name) == POISON).all() for name in ("atable", "ahist", "acounts", "labels"))
        finally:
            d.free()
