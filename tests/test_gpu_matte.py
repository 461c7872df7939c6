"""Matte and Composite on the GPU against tests/matte_ref.py: exact integers, so every comparison is ``==`` on whole arrays, on
poisoned device buffers with guard bytes behind them (``Dev`` of tests/test_gpu_anchors.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Composite, CompositeCmd, CompositeOut, FramePath, Matte, MatteCmd, MatteOut

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matte_ref as M  # noqa: E402
from test_gpu_anchors import POISON, Dev  # noqa: E402

pytestmark = pytest.mark.gpu

TH, TW = _lib.MATTE_TILE_H, _lib.MATTE_TILE_W
# one pixel; less than a wave; one pixel past a tile either way; the issue's plane (4 x 2 tiles); two tiles by two, ragged
SHAPES = ((1, 1), (5, 7), (TH + 1, TW + 1), (61, 97), (2 * TH - 3, 2 * TW - 27))
WINDOWS = ((1, 1), (3, 12), (8, 24), (16, 255))
SELECT = np.array([0, 0, 0, 1, 0], np.uint8)  # value 3 of five rows


def scene(h, w, dtype=np.uint8, seed=0):
    """a disc in the picture that leaves the frame, with a little noise; the plane holds the same disc quantised to 8 x 8 blocks
    (value 3 inside, 1 outside), so its border follows no edge of the picture and crosses tile seams and the frame's border; a
    patch of a value beyond the table; a confidence plane"""
    rng = np.random.default_rng(seed + h * w)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = lambda y, x: (y - 0.45 * h) ** 2 + (x - 0.55 * w) ** 2 < (0.6 * max(min(h, w), 8)) ** 2  # noqa: E731
    frame = np.where(disc(yy, xx)[..., None], [200, 150, 90], [30, 60, 120]).astype(np.uint8) + rng.integers(0, 16, (h, w, 3), dtype=np.uint8)
    plane = np.where(disc(yy // 8 * 8 + 4, xx // 8 * 8 + 4), 3, 1).astype(dtype)
    plane[h // 2:h // 2 + 3, :w // 3] = np.iinfo(dtype).max
    return frame, plane, rng.integers(0, 256, (h, w), dtype=np.uint8)


def dev_matte(ctx, frame, plane, select, flags, conf, radius, sigma, want=("alpha", "counts"), d=None):
    """infur_matte_dev on poisoned, guarded buffers -> (alpha, counts), None where not wanted (checked untouched)"""
    h, w = plane.shape
    own = d is None
    d = d or Dev(ctx, frame=frame.nbytes, plane=plane.nbytes, select=select.size, conf=h * w, alpha=h * w, counts=32)
    try:
        d.poison("alpha", "counts")
        for name, a in (("frame", frame), ("plane", plane), ("select", select), ("conf", conf)):
            d.put(name, a)
        ctx.check(ctx.L.infur_matte_dev(ctx.h, d.ptr["frame"], d.ptr["plane"], plane.dtype.itemsize, h, w, d.ptr["select"], select.size, flags,
                                        d.ptr["conf"] if flags & M.CONF else None, radius, sigma, d.ptr["alpha"] if "alpha" in want else None,
                                        d.ptr["counts"] if "counts" in want else None))
        ctx.synchronize()
        alpha, counts = d.get("alpha").reshape(h, w), d.get("counts").view(np.uint32)  # (get checks the guard behind h * w)
        assert "alpha" in want or (alpha == POISON).all(), "alpha was not wanted and was written"
        assert "counts" in want or (counts.view(np.uint8) == POISON).all(), "counts were not wanted and were written"
        return alpha if "alpha" in want else None, counts if "counts" in want else None
    finally:
        if own:
            d.free()


@pytest.mark.parametrize("window", WINDOWS, ids=lambda v: f"r{v[0]}s{v[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_alpha_and_counts_equal_the_rule(ctx, shape, window):
    assert ctx.L.infur_features() & _lib.FEATURE_MATTE  # (fails on a library without the feature)
    (h, w), (radius, sigma) = shape, window
    for dtype, flags in ((np.uint8, 0), (np.uint32, M.INVERT), (np.uint8, M.CONF), (np.uint32, M.CONF | M.INVERT)):
        frame, plane, conf = scene(h, w, dtype)
        ref_alpha, ref_counts = M.matte(frame, plane, SELECT, radius, sigma, flags, conf)
        alpha, counts = dev_matte(ctx, frame, plane, SELECT, flags, conf, radius, sigma)
        assert (counts == ref_counts).all(), (flags, counts, ref_counts)
        assert (alpha == ref_alpha).all(), (flags, np.argwhere(alpha != ref_alpha)[:4])
        assert counts[2:5].sum() == h * w and (ref_counts[M.C_OUTSIDE] or h < 3)
        assert dev_matte(ctx, frame, plane, SELECT, flags, conf, radius, sigma, want=("alpha",))[0].tobytes() == alpha.tobytes()
        assert dev_matte(ctx, frame, plane, SELECT, flags, conf, radius, sigma, want=("counts",))[1].tobytes() == counts.tobytes()


def test_the_sums_need_all_32_bits(ctx):
    """every full window holds one 254 among 255s, so no shortcut applies: N = 4096 (1088 * 255 + 254), 2N + D = 2 279 329 792 > 2^31"""
    frame, plane, conf = np.full((67, 67, 3), 9, np.uint8), np.zeros((67, 67), np.uint8), np.full((67, 67), 255, np.uint8)
    conf[::33, ::33] = 254
    assert (M.matte(frame, plane, [1], 16, 255, M.CONF, conf)[0] == 255).all()
    alpha, counts = dev_matte(ctx, frame, plane, np.ones(1, np.uint8), M.CONF, conf, 16, 255)
    assert (alpha == 255).all() and counts.tolist() == [67 * 67, 0, 0, 0, 67 * 67, 0, 0, 0]


def test_quiet_windows(ctx):
    """one selected square well inside: alpha is 0 or 255 wherever the window sees one value, and the rule everywhere"""
    h, w, r = 3 * TH + 5, 2 * TW + 9, 3
    frame, plane, conf = scene(h, w, seed=1)
    plane[:] = 1
    plane[20:34, 60:90] = 3
    alpha, counts = dev_matte(ctx, frame, plane, SELECT, 0, conf, r, 12)
    ref_alpha, ref_counts = M.matte(frame, plane, SELECT, r, 12)
    assert (alpha == ref_alpha).all() and (counts == ref_counts).all()
    yy, xx = np.mgrid[0:h, 0:w]
    assert not alpha[(yy < 20 - r) | (yy >= 34 + r) | (xx < 60 - r) | (xx >= 90 + r)].any()
    assert (alpha[20 + r:34 - r, 60 + r:90 - r] == 255).all() and counts[M.C_SOFT]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "odd addresses"])
@pytest.mark.parametrize("shape", [(5, 7), (6, 10), (61, 97)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", [M.COLOUR, M.IMAGE, M.CUTOUT])
def test_composite(ctx, mode, shape, shift):
    """out of place and in place; 35, 60 and 5917 pixels: ragged ends and none; word loads and, at odd addresses, bytes"""
    (h, w), rng = shape, np.random.default_rng(7)
    frame, back = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, (h, w), dtype=np.uint8)
    alpha.ravel()[:6] = [0, 1, 127, 128, 254, 255]
    ref = M.composite(frame, alpha, mode, back, 0x0A6432)
    pad = lambda a: np.concatenate([np.full(shift, POISON, np.uint8), a.ravel(), np.full(4 - shift, POISON, np.uint8)])  # noqa: E731
    d = Dev(ctx, frame=frame.nbytes + 4, alpha=alpha.nbytes + 4, back=back.nbytes + 4, out=ref.nbytes + 4)
    try:
        at = {name: C.c_void_p(p.value + shift) for name, p in d.ptr.items()}
        for in_place in ((False, True) if mode != M.CUTOUT else (False,)):
            d.poison("out")
            for name, a in (("frame", frame), ("alpha", alpha), ("back", back)):
                d.put(name, pad(a))
            out = "frame" if in_place else "out"
            ctx.check(ctx.L.infur_composite_dev(ctx.h, at["frame"], at["alpha"], h, w, mode, at["back"] if mode == M.IMAGE else None, 0x0A6432, at[out]))
            ctx.synchronize()
            assert d.get(out).tobytes() == pad(ref).tobytes(), (in_place, "the picture, or the bytes around it")
            assert in_place or d.get("frame").tobytes() == pad(frame).tobytes()
    finally:
        d.free()
    if not shift:  # the host-pointer call and the processor
        res = CompositeOut()
        Composite(ctx, CompositeCmd(mode, (0x32, 0x64, 0x0A))).advance((frame, alpha, back if mode == M.IMAGE else None), res)
        assert res.out.tobytes() == ref.tobytes()


@pytest.mark.parametrize("factor", [1.0, 0.5])
@pytest.mark.parametrize("mode", [M.IMAGE, M.CUTOUT])
def test_frame_calls_equal_segments_then_matte_then_composite(ctx, model, mode, factor):
    L, fp, (h, w) = ctx.L, FramePath(ctx), (48, 64)
    frame = W.synth_frame(h, w, index=5)
    seg = fp.advance_segments(frame, factor, _lib.DECODE_RAW, want_scaled=True, want_conf=True)
    (oh_, ow_), ch = seg.klass.shape, 4 if mode == M.CUTOUT else 3
    npix = oh_ * ow_
    cmd = MatteCmd([int(seg.klass[0, 0]), int(seg.klass[oh_ // 2, ow_ // 2])], radius=3, sigma=24, use_conf=True)
    table, back = cmd.table(), np.random.default_rng(1).integers(0, 256, (oh_, ow_, 3), dtype=np.uint8)
    ref_alpha, ref_counts = M.matte(seg.scaled, seg.klass, table, 3, 24, cmd.flags(), seg.conf)
    ref = M.composite(seg.scaled, ref_alpha, mode, back)
    d = Dev(ctx, bgr=frame.nbytes, select=table.size, back=back.nbytes, klass=npix, conf=npix, scaled=npix * 3, alpha=npix, composed=npix * ch, counts=32)
    try:
        P, ow, oh = d.ptr, C.c_uint32(0), C.c_uint32(0)
        for name, a in (("bgr", frame), ("select", table), ("back", back)):
            d.put(name, a)
        ctx.check(L.infur_frame_segments_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, P["klass"], P["conf"], npix, None, 0, None, 0, P["scaled"],
                                             C.byref(ow), C.byref(oh)))
        ctx.check(L.infur_matte_dev(ctx.h, P["scaled"], P["klass"], 1, oh.value, ow.value, P["select"], table.size, cmd.flags(), P["conf"], 3, 24,
                                    P["alpha"], P["counts"]))
        ctx.check(L.infur_composite_dev(ctx.h, P["scaled"], P["alpha"], oh.value, ow.value, mode, P["back"], 0, P["composed"]))
        ctx.synchronize()
        chain = d.get("alpha"), d.get("composed"), d.get("counts")
        assert chain[0].tobytes() == ref_alpha.tobytes() and chain[1].tobytes() == ref.tobytes() and chain[2].tobytes() == ref_counts.tobytes()
        for alone in (False, True):  # every output; then the composed frame alone: the planes go to the library's scratch
            d.poison("alpha", "composed", "counts", "klass", "conf", "scaled")
            ctx.check(L.infur_frame_matte_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, P["select"], table.size, cmd.flags(), 3, 24, mode, P["back"],
                                              0, None if alone else P["alpha"], P["composed"], npix * ch, None if alone else P["klass"],
                                              None if alone else P["conf"], npix, None if alone else P["counts"], None if alone else P["scaled"],
                                              C.byref(ow), C.byref(oh)))
            ctx.synchronize()
            assert d.get("composed").tobytes() == chain[1].tobytes()
            if alone:
                assert all((d.get(name) == POISON).all() for name in ("alpha", "counts", "klass", "conf", "scaled"))
            else:
                assert d.get("alpha").tobytes() == chain[0].tobytes() and d.get("counts").tobytes() == chain[2].tobytes()
                assert d.get("klass").tobytes() == seg.klass.tobytes() and d.get("conf").tobytes() == seg.conf.tobytes()
        assert L.infur_frame_matte_dev(ctx.h, P["bgr"], w, h, factor, 0, _lib.DECODE_RAW, P["select"], table.size, 0, 3, 24, mode, P["back"], 0, None,
                                       P["composed"], npix * ch - 1, None, None, 0, None, None, C.byref(ow), C.byref(oh)) == _lib.E_CAPACITY
    finally:
        d.free()
    r = fp.advance_matte(frame, cmd, CompositeCmd(mode), back, factor, want_klass=True, want_conf=True, want_scaled=True)  # host pointers
    assert r.alpha.tobytes() == chain[0].tobytes() and r.composed.tobytes() == chain[1].tobytes() and r.counts.tobytes() == chain[2].tobytes()
    assert (r.klass == seg.klass).all() and (r.conf == seg.conf).all() and (r.scaled == seg.scaled).all()


def test_rejected_calls_and_the_next_valid_one(ctx):
    L, (frame, plane, conf) = ctx.L, scene(6, 7)
    d = Dev(ctx, frame=frame.nbytes, plane=plane.nbytes, select=5, conf=42, alpha=42, counts=32, out=frame.nbytes)
    try:
        P = d.ptr
        matte = lambda fr=P["frame"], pl=P["plane"], elem=1, hh=6, ww=7, sel=P["select"], rows=5, flags=0, cf=P["conf"], radius=2, sigma=12, alpha=P["alpha"], counts=P["counts"]: (  # noqa: E731
            L.infur_matte_dev(ctx.h, fr, pl, elem, hh, ww, sel, rows, flags, cf, radius, sigma, alpha, counts))
        comp = lambda fr=P["frame"], al=P["alpha"], hh=6, ww=7, mode=M.COLOUR, back=None, out=P["out"]: (  # noqa: E731
            L.infur_composite_dev(ctx.h, fr, al, hh, ww, mode, back, 0, out))
        for call, kw, message in ((matte, dict(elem=2), "elem_bytes"), (matte, dict(flags=4), "unknown matte flags"), (matte, dict(radius=0), "radius 0: 1 to 16"),
                                  (matte, dict(radius=17), "radius 17: 1 to 16"), (matte, dict(sigma=0), "sigma 0: 1 to 255"),
                                  (matte, dict(sigma=256), "sigma 256: 1 to 255"), (matte, dict(hh=0), "1 to 32768"), (matte, dict(sel=None), "no select pointer"),
                                  (matte, dict(alpha=None, counts=None), "no output wanted"), (matte, dict(pl=None), "no plane pointer"),
                                  (matte, dict(fr=None), "no frame pointer"), (matte, dict(flags=M.CONF, cf=None), "INFUR_MATTE_CONF and no conf"),
                                  (comp, dict(mode=3), "unknown composite mode 3"), (comp, dict(ww=32769), "1 to 32768"), (comp, dict(al=None), "no alpha pointer"),
                                  (comp, dict(out=None), "no output wanted"), (comp, dict(mode=M.IMAGE), "INFUR_COMPOSITE_IMAGE and no back"),
                                  (comp, dict(out=C.c_void_p(P["frame"].value + 3)), "overlaps the frame"),
                                  (comp, dict(mode=M.CUTOUT, out=P["frame"]), "overlaps the frame")):
            assert call(**kw) == _lib.E_INVALID_ARG and message in ctx.last_error(), (kw, ctx.last_error())
        for name, a in (("frame", frame), ("plane", plane), ("select", SELECT), ("conf", conf)):
            d.put(name, a)
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("alpha", "counts", "out"))
        assert matte(flags=M.CONF) == comp() == _lib.OK  # the next valid calls
        ctx.synchronize()
        ref_alpha = M.matte(frame, plane, SELECT, 2, 12, M.CONF, conf)[0]
        assert (d.get("alpha").reshape(6, 7) == ref_alpha).all() and d.get("out").tobytes() == M.composite(frame, ref_alpha, M.COLOUR).tobytes()
    finally:
        d.free()


def test_the_same_bytes_after_other_stages_and_from_the_processor(ctx):
    frame, plane, conf = scene(61, 97, np.uint32)
    first = dev_matte(ctx, frame, plane, SELECT, M.CONF, conf, 8, 24)
    big = scene(3 * TH, 3 * TW)
    assert (dev_matte(ctx, *big[:2], SELECT, 0, big[2], 16, 3)[0] == M.matte(*big[:2], SELECT, 16, 3)[0]).all()  # another sigma's weights in between
    res = MatteOut()
    Matte(ctx, MatteCmd(SELECT, 8, 24, use_conf=True)).advance((frame, plane, conf), res)  # infur_matte, host pointers
    again = dev_matte(ctx, frame, plane, SELECT, M.CONF, conf, 8, 24)
    assert first[0].tobytes() == again[0].tobytes() == res.alpha.tobytes() and first[1].tobytes() == again[1].tobytes() == res.counts.tobytes()
