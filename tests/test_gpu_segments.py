"""Segments on the GPU: class plane, confidence plane, per-class statistics and the overlay shaded by that confidence -- unfused
(``Segments`` over [K,H,W]) and fused into the up-sampling kernel (``FramePath.advance_segments``) -- against the C oracle
(RAW) and tests/segments_ref.py (SOFTMAX, statistics)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, InfurError, Model, ModelCmd, Segments, SegmentsOut, class_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX


def run(ctx, x, decode, **want):
    out = SegmentsOut(want_klass=True, want_conf=True, want_stats=True, want_rgba=True) if not want else SegmentsOut(**want)
    Segments(ctx, decode).advance(x, out)
    return out


def crafted(rng, k, h, w):
    x = rng.normal(0.4, 0.5, size=(k, h, w)).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = np.nan
    x[rng.random(x.shape) < 0.01] = np.inf
    x[rng.random(x.shape) < 0.01] = -np.inf
    return x


# --------------------------------------------------------------------------- #
# 1. unfused, RAW
# --------------------------------------------------------------------------- #
def test_unfused_raw_equals_the_oracle(ctx, oracle):
    assert ctx.L.infur_features() & _lib.FEATURE_SEGMENTS  # (the first line: fails on a library without the feature)
    rng = np.random.default_rng(5)
    for k, h, w in ((21, 33, 47), (1, 4, 4), (22, 24, 32), (40, 7, 9), (21, 270, 480)):
        x = crafted(rng, k, h, w)
        if k == 21:
            x[13] = -1.0  # an absent class
        o = run(ctx, x, RAW)
        kl, cf = oracle.argmax(x)
        assert (o.klass == kl).all() and (o.conf == cf).all(), (k, h, w)
        assert (o.rgba == oracle.colorcode(x)).all(), (k, h, w)
        st = R.stats(kl, cf, k)
        assert o.stats.shape == (k, 8) and (o.stats == st).all(), (k, h, w, o.stats, st)
        if k == 21:
            assert o.stats[13].tolist() == [0, 0, 0, 0, int(R.U64_MAX), int(R.U64_MAX), 0, 0]
    # the statistics accumulate nothing across calls
    o2 = run(ctx, x, RAW)
    assert (o2.stats == st).all()


def test_unfused_rules_and_error_codes(ctx, oracle):
    L, h = ctx.L, ctx.h
    x = np.random.default_rng(1).normal(0.3, 0.5, size=(5, 6, 7)).astype(np.float32)
    kl, cf, rgba = np.full((6, 7), 9, np.uint8), np.full((6, 7), 9, np.uint8), np.full((6, 7, 4), 9, np.uint8)
    st = np.full((5, 8), 9, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    # reported before any work: unknown decode mode, more classes than the class byte holds
    assert L.infur_segments(h, p(x), 5, 6, 7, 2, p(kl), p(cf), p(st), p(rgba)) == _lib.E_INVALID_ARG
    assert L.infur_segments(h, p(x), 257, 6, 7, 0, p(kl), p(cf), p(st), p(rgba)) == _lib.E_INVALID_ARG
    assert L.infur_segments(h, p(x), 257, 0, 7, 0, p(kl), p(cf), p(st), p(rgba)) == _lib.E_INVALID_ARG
    assert (kl == 9).all() and (st == 9).all() and (rgba == 9).all()
    # all outputs NULL; a NULL input with k > 0
    assert L.infur_segments(h, p(x), 5, 6, 7, 0, None, None, None, None) == _lib.E_INVALID_ARG
    assert L.infur_segments(h, None, 5, 6, 7, 0, p(kl), None, None, None) == _lib.E_INVALID_ARG
    # an empty image is OK and writes nothing
    assert L.infur_segments(h, p(x), 5, 0, 7, 0, p(kl), p(cf), p(st), p(rgba)) == _lib.OK
    assert L.infur_segments(h, p(x), 5, 6, 0, 1, None, None, None, None) == _lib.OK
    assert (kl == 9).all() and (cf == 9).all() and (st == 9).all() and (rgba == 9).all()
    # k == 0: zero planes, infur_colorcode's rgba, stats untouched
    for mode in (RAW, SOFTMAX):
        kl[:], cf[:], rgba[:], st[:] = 9, 9, 9, 9
        assert L.infur_segments(h, None, 0, 6, 7, mode, p(kl), p(cf), p(st), p(rgba)) == _lib.OK
        assert (kl == 0).all() and (cf == 0).all() and (st == 9).all()
        ref = np.empty((6, 7, 4), np.uint8)
        assert L.infur_colorcode(h, None, 0, 6, 7, p(ref)) == _lib.OK
        assert (rgba == ref).all()
    # 256 classes is the most the class byte holds: it runs, and class 255 can win
    big = np.zeros((256, 3, 5), np.float32)
    big[255, 1, :] = 0.75
    o = run(ctx, big, RAW)
    assert (o.klass[1] == 255).all() and (o.klass[0] == 0).all() and o.stats[255, R.PIXELS] == 5 and o.stats[255, R.MIN_Y] == 1
    with pytest.raises(InfurError):
        Segments(ctx).control(7)


def test_outputs_stay_inside_their_buffers(ctx, oracle):
    """64 poisoned guard bytes behind each device output survive; so does everything behind a 3-column image's byte rows"""
    L, h = ctx.L, ctx.h
    rng = np.random.default_rng(2)
    for k, hh, ww in ((21, 33, 47), (21, 16, 64), (3, 5, 3)):
        x = crafted(rng, k, hh, ww)
        hw = hh * ww
        sizes = {"klass": hw, "conf": hw, "stats": k * 64, "rgba": hw * 4}
        dev = {}
        for name, n in list(sizes.items()) + [("x", x.nbytes)]:
            d = C.c_void_p(None)
            ctx.check(L.infur_dev_alloc(h, n + 64, C.byref(d)))
            poison = np.full(n + 64, 0xA5, np.uint8)
            ctx.check(L.infur_memcpy_h2d(h, d, poison.ctypes.data, n + 64))
            dev[name] = d
        ctx.check(L.infur_memcpy_h2d(h, dev["x"], x.ctypes.data, x.nbytes))
        for mode in (RAW, SOFTMAX):
            ctx.check(L.infur_segments_dev(h, dev["x"], k, hh, ww, mode, dev["klass"], dev["conf"], dev["stats"], dev["rgba"]))
            ctx.synchronize()
            got = {}
            for name, n in sizes.items():
                b = np.empty(n + 64, np.uint8)
                ctx.check(L.infur_memcpy_d2h(h, b.ctypes.data, dev[name], n + 64))
                assert (b[n:] == 0xA5).all(), (name, k, hh, ww, mode)
                got[name] = b[:n]
            if mode == RAW:
                kl, cf = oracle.argmax(x)
                assert (got["klass"] == kl.ravel()).all() and (got["conf"] == cf.ravel()).all()
                assert (got["stats"].view(np.uint64).reshape(k, 8) == R.stats(kl, cf, k)).all()
        for d in dev.values():
            ctx.check(L.infur_dev_free(h, d))


# --------------------------------------------------------------------------- #
# 2. unfused, SOFTMAX
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("k", [21, 22])
@pytest.mark.parametrize("sigma", [1.0, 2.0, 4.0])
def test_unfused_softmax(ctx, tables, sigma, k):
    x = np.random.default_rng(5).normal(0.0, sigma, size=(k, 500, 400)).astype(np.float32)  # the inputs of the CPU band test
    o = run(ctx, x, SOFTMAX)
    kl, cf = R.decode(x, R.SOFTMAX)
    band = R.in_band(x)
    assert band.mean() <= 0.01
    assert (o.klass == kl).all()
    diff = o.conf.astype(int) - cf.astype(int)
    print(f"sigma {sigma} K {k}: {int((diff != 0).sum())} of {diff.size} confidence bytes differ, {int(band.sum())} pixels in the band")
    assert (diff[~band] == 0).all(), "a confidence byte differs outside the band"
    assert (np.abs(diff) <= 1).all()
    st = R.stats(kl, cf, k)
    cols = [R.PIXELS, R.SUM_X, R.SUM_Y, R.MIN_X, R.MIN_Y, R.MAX_X, R.MAX_Y]
    assert (o.stats[:, cols] == st[:, cols]).all()
    in_band_per_class = np.bincount(kl[band].ravel(), minlength=k)
    assert (np.abs(o.stats[:, R.SUM_CONF].astype(np.int64) - st[:, R.SUM_CONF].astype(np.int64)) <= in_band_per_class).all()
    assert (o.stats == R.stats(o.klass, o.conf, k)).all()  # ... and exact for the kernel's own planes
    assert (o.rgba == tables["color_lut"][o.klass % 20, o.conf]).all()


def test_unfused_softmax_non_finite(ctx, tables):
    inf, nan = np.inf, np.nan
    px = np.array([
        [nan, nan, nan],        # nothing wins: class 0, conf 0
        [-inf, -inf, -inf],     # the same
        [1.0, inf, 2.0],        # +inf: class 1, conf 255
        [nan, -3.0, nan],       # NaN beside a finite maximum: class 1, p = 1
        [-2.0, -2.0, -5.0],     # negative maxima; the first maximum wins
        [0.0, 0.0, 0.0],        # p = 1/3 -> 85
        [-inf, 7.0, -inf],      # -inf terms contribute 0
        [inf, inf, nan],        # two +inf: the first
    ], np.float32).T.reshape(3, 1, 8)
    x = np.tile(px, (1, 5, 9))  # 72 columns: more than one tile wide
    o = run(ctx, x, SOFTMAX)
    kl, cf = R.decode(x, R.SOFTMAX)
    assert kl[0, :8].tolist() == [0, 0, 1, 1, 0, 0, 1, 0] and cf[0, [0, 1, 2, 3, 5, 6, 7]].tolist() == [0, 0, 255, 255, 85, 255, 255]
    assert (o.klass == kl).all() and (o.conf == cf).all()
    assert (o.stats == R.stats(kl, cf, 3)).all()
    assert (o.rgba == tables["color_lut"][o.klass % 20, o.conf]).all()
    # 40 classes (beyond a staged slot), negative everywhere: RAW answers class 0 / conf 0, SOFTMAX finds the maximum
    y = -np.abs(np.random.default_rng(3).normal(2.0, 1.0, size=(40, 9, 70))).astype(np.float32) - 0.01
    o = run(ctx, y, SOFTMAX)
    kl, cf = R.decode(y, R.SOFTMAX)
    band = R.in_band(y)
    assert (o.klass == kl).all() and (o.klass == y.argmax(axis=0)).all()
    assert (o.conf[~band] == cf[~band]).all() and (np.abs(o.conf.astype(int) - cf.astype(int)) <= 1).all()
    r = run(ctx, y, RAW)
    assert (r.klass == 0).all() and (r.conf == 0).all() and r.stats[0, R.PIXELS] == 9 * 70


# --------------------------------------------------------------------------- #
# 3. fused vs oracle, RAW
# --------------------------------------------------------------------------- #
def fused_raw_case(ctx, model, oracle, frame, factor, mode, k):
    fp = FramePath(ctx, scale_mode=mode)
    s = fp.advance_segments(frame, factor, RAW, want_rgba=True, want_scaled=True)
    lo, _ = model.lowres()  # the run's own low-res logits: the decode is what is checked here, not the conv stack
    oh, ow = s.scaled.shape[:2]
    assert s.klass.shape == (oh, ow) and s.conf.shape == (oh, ow) and s.stats.shape == (k, 8) and s.rgba.shape == (oh, ow, 4)
    kl, cf = oracle.argmax(oracle.upsample_bilinear(lo, oh, ow))
    assert (s.klass == kl).all() and (s.conf == cf).all(), (frame.shape, factor, mode)
    assert (s.stats == R.stats(kl, cf, k)).all(), (frame.shape, factor, mode)
    rgba, scaled = fp.advance(frame, factor, want_scaled=True)
    assert (s.rgba == rgba).all() and (s.scaled == scaled).all(), (frame.shape, factor, mode)
    lo2, _ = model.lowres()
    assert (lo.view(np.uint32) == lo2.view(np.uint32)).all()
    return s


def test_fused_raw_equals_the_oracle(ctx, model, oracle):
    k = model.get_info().num_classes
    for h, w in ((61, 97), (240, 320), (1080, 1920)):
        frame = W.synth_frame(h, w, index=h)
        for factor in (1.0, 0.5):
            for mode in (_lib.SCALE_NEAREST, _lib.SCALE_BILINEAR):
                s = fused_raw_case(ctx, model, oracle, frame, factor, mode, k)
    recs = class_summary(s.stats, s.klass.shape[1], s.klass.shape[0])
    assert sum(r["pixels"] for r in recs) == s.klass.size and abs(sum(r["share"] for r in recs) - 1.0) < 1e-9
    assert all(r["box"][0] <= r["centroid"][0] <= r["box"][2] and r["box"][1] <= r["centroid"][1] <= r["box"][3] for r in recs)


def test_fused_raw_f16hl_and_quantised(oracle, blob50):
    from oracle import infur_qoracle as Q

    frame = W.synth_frame(240, 320, index=4)
    with Context(device=0, dtype="f16hl") as c:
        m = Model(c).control(ModelCmd.LoadBlob(blob50))
        fused_raw_case(c, m, oracle, frame, 1.0, _lib.SCALE_NEAREST, m.get_info().num_classes)
    with Context(device=0) as c:
        m = Model(c).control(ModelCmd.LoadBlob(Q.synth_qblob()))
        assert m.get_info().quantised
        fused_raw_case(c, m, oracle, frame, 0.5, _lib.SCALE_BILINEAR, m.get_info().num_classes)


def test_fused_rules_and_error_codes(ctx, model, blob50):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    k = model.get_info().num_classes
    kl, cf, rgba = np.zeros((48, 64), np.uint8), np.zeros((48, 64), np.uint8), np.zeros((48, 64, 4), np.uint8)
    st = np.zeros((k, 8), np.uint64)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(decode=0, klass=kl, conf=cf, plane_cap=48 * 64, stats=st, classes=k, mask=rgba, mask_cap=48 * 64 * 4, mode=0, factor=1.0):
        return L.infur_frame_segments(h, p(frame), 64, 48, factor, mode, decode, p(klass) if klass is not None else None,
                                      p(conf) if conf is not None else None, plane_cap, p(stats) if stats is not None else None, classes,
                                      p(mask) if mask is not None else None, mask_cap, None, C.byref(ow), C.byref(oh))

    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48)
    assert call(decode=2) == _lib.E_INVALID_ARG
    assert call(mode=2) == _lib.E_INVALID_ARG
    assert call(klass=None, conf=None, stats=None, mask=None) == _lib.E_INVALID_ARG
    assert call(plane_cap=48 * 64 - 1) == _lib.E_CAPACITY
    assert call(klass=None, conf=None, plane_cap=0) == _lib.OK  # no plane wanted: its capacity does not matter
    assert call(mask_cap=48 * 64 * 4 - 1) == _lib.E_CAPACITY
    assert call(classes=k - 1) == _lib.E_CAPACITY
    assert call(factor=-1.0) == _lib.E_INVALID_SCALE
    # the launch is recorded under a stable kernel name
    with Context(device=0, profile=True) as c:
        Model(c).control(ModelCmd.LoadBlob(blob50))
        FramePath(c).advance_segments(frame, 0.5, SOFTMAX)
        prof = c.profile()
        assert [r["kernel"] for r in prof].count("upsample_argmax_segments") == 1 and prof[-1]["kernel"] == "upsample_argmax_segments"
        assert prof[0]["kernel"].startswith("scale") and not any(r["kernel"] == "upsample_argmax_shade" for r in prof)
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        s = FramePath(c).advance_segments(frame, 0.5, RAW, want_scaled=True)
        assert s.klass is None and s.stats is None and s.scaled.shape == (24, 32, 3)
        rc = c.L.infur_frame_segments(c.h, p(frame), 64, 48, 1.0, 0, 0, p(kl), None, 48 * 64, None, 0, None, 0, None, C.byref(ow), C.byref(oh))
        assert rc == _lib.E_MODEL_NOT_LOADED


def test_fused_outputs_stay_inside_their_buffers(ctx, model):
    """the fused kernel stores the byte planes as dwords gathered from four lanes (100 columns) or as bytes (99 columns); 52 / 50
    rows end inside a 16-row tile: the 64 poisoned bytes behind every output survive"""
    L, h = ctx.L, ctx.h
    k = model.get_info().num_classes
    for hh, ww in ((52, 100), (50, 99)):
        frame = W.synth_frame(hh, ww, index=2)
        hw = hh * ww
        sizes = {"klass": hw, "conf": hw, "stats": k * 64, "rgba": hw * 4}
        dev = {}
        for name, n in list(sizes.items()) + [("bgr", frame.nbytes)]:
            d = C.c_void_p(None)
            ctx.check(L.infur_dev_alloc(h, n + 64, C.byref(d)))
            poison = np.full(n + 64, 0xA5, np.uint8)
            ctx.check(L.infur_memcpy_h2d(h, d, poison.ctypes.data, n + 64))
            dev[name] = d
        ctx.check(L.infur_memcpy_h2d(h, dev["bgr"], frame.ctypes.data, frame.nbytes))
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        for mode in (RAW, SOFTMAX):
            ctx.check(L.infur_frame_segments_dev(h, dev["bgr"], ww, hh, 1.0, 0, mode, dev["klass"], dev["conf"], hw, dev["stats"], k, dev["rgba"],
                                                 hw * 4, None, C.byref(ow), C.byref(oh)))
            ctx.synchronize()
            got = {}
            for name, n in sizes.items():
                b = np.empty(n + 64, np.uint8)
                ctx.check(L.infur_memcpy_d2h(h, b.ctypes.data, dev[name], n + 64))
                assert (b[n:] == 0xA5).all(), (name, hh, ww, mode)
                got[name] = b[:n]
            s = FramePath(ctx).advance_segments(frame, 1.0, mode, want_rgba=True)
            assert (got["klass"] == s.klass.ravel()).all() and (got["conf"] == s.conf.ravel()).all()
            assert (got["stats"].view(np.uint64).reshape(k, 8) == s.stats).all() and (got["rgba"] == s.rgba.ravel()).all()
        for d in dev.values():
            ctx.check(L.infur_dev_free(h, d))


@pytest.mark.parametrize("ow", [8, 12, 7])  # OW % 4 == 0: the fused kernel's dword row stores when the planes are dword-aligned
def test_planes_at_unaligned_device_pointers(ctx, model, oracle, ow):
    """include/infur_hip.h: a device pointer needs only the natural alignment of its element type -- a byte plane may start anywhere.
    klass / conf at byte offsets 0..3 (each on its own, and both): the planes equal the oracle's, and the bytes before them and the
    64 guard bytes behind every output still hold the poison"""
    from test_gpu_parity import GuardedDev

    L, h = ctx.L, ctx.h
    k = model.get_info().num_classes
    oh = 5
    x = crafted(np.random.default_rng(ow), k, oh, ow)
    kl, cf = oracle.argmax(x)
    frame = W.synth_frame(oh, ow, index=3)
    aligned = FramePath(ctx).advance_segments(frame, 1.0, RAW, want_rgba=True)
    lo, _ = model.lowres()
    fkl, fcf = oracle.argmax(oracle.upsample_bilinear(lo, oh, ow))
    assert (aligned.klass == fkl).all() and (aligned.conf == fcf).all()
    hw = oh * ow
    d_x, d_bgr = GuardedDev(ctx, x.nbytes, 0, x), GuardedDev(ctx, frame.nbytes, 0, frame)
    for k_off, c_off in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 3), (3, 2)):
        what = (ow, k_off, c_off)
        # unfused
        d_kl, d_cf, d_st, d_rgba = GuardedDev(ctx, hw, k_off), GuardedDev(ctx, hw, c_off), GuardedDev(ctx, k * 64, 0), GuardedDev(ctx, hw * 4, 0)
        ctx.check(L.infur_segments_dev(h, d_x.ptr, k, oh, ow, RAW, d_kl.ptr, d_cf.ptr, d_st.ptr, d_rgba.ptr))
        ctx.synchronize()
        assert (d_kl.read(what) == kl.ravel()).all() and (d_cf.read(what) == cf.ravel()).all(), what
        assert (d_st.read(what).view(np.uint64).reshape(k, 8) == R.stats(kl, cf, k)).all(), what
        assert (d_rgba.read(what) == oracle.colorcode(x).ravel()).all(), what
        for d in (d_kl, d_cf, d_st, d_rgba):
            d.free()
        # fused into the up-sampling kernel
        d_kl, d_cf, d_st, d_rgba = GuardedDev(ctx, hw, k_off), GuardedDev(ctx, hw, c_off), GuardedDev(ctx, k * 64, 0), GuardedDev(ctx, hw * 4, 0)
        rw, rh = C.c_uint32(0), C.c_uint32(0)
        ctx.check(L.infur_frame_segments_dev(h, d_bgr.ptr, ow, oh, 1.0, 0, RAW, d_kl.ptr, d_cf.ptr, hw, d_st.ptr, k, d_rgba.ptr, hw * 4, None,
                                             C.byref(rw), C.byref(rh)))
        ctx.synchronize()
        assert (rw.value, rh.value) == (ow, oh)
        assert (d_kl.read(what) == fkl.ravel()).all() and (d_cf.read(what) == fcf.ravel()).all(), what
        assert (d_st.read(what).view(np.uint64).reshape(k, 8) == R.stats(fkl, fcf, k)).all(), what
        assert (d_rgba.read(what) == aligned.rgba.ravel()).all(), what
        for d in (d_kl, d_cf, d_st, d_rgba):
            d.free()
    d_x.free()
    d_bgr.free()


# --------------------------------------------------------------------------- #
# 4. fused == unfused (a self-comparison: the link to the oracle is tests 1-3)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_equals_unfused(ctx, model, decode):
    for h, w in ((240, 320), (540, 960)):
        frame = W.synth_frame(h, w, index=w)
        s = FramePath(ctx).advance_segments(frame, 1.0, decode, want_rgba=True)
        outs = []
        model.advance(frame, outs)  # full-resolution logits through upsample_planar
        o = run(ctx, outs[0], decode)
        assert (s.klass == o.klass).all() and (s.conf == o.conf).all() and (s.rgba == o.rgba).all() and (s.stats == o.stats).all()
        if decode == SOFTMAX:
            assert (s.klass == outs[0].argmax(axis=0)).all()


# --------------------------------------------------------------------------- #
# 5. subsets
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_each_output_alone_equals_all_together(ctx, model, decode):
    frame = W.synth_frame(122, 164, index=6)  # 164 columns: 4-byte rows; and 0.5 -> 82 columns: byte stores
    for factor in (1.0, 0.5):
        fp = FramePath(ctx)
        full = fp.advance_segments(frame, factor, decode, want_rgba=True)
        outs = []
        model.advance(frame, outs)
        ufull = run(ctx, outs[0], decode)
        for name in ("klass", "conf", "stats", "rgba"):
            want = {f"want_{n}": n == name for n in ("klass", "conf", "stats", "rgba")}
            one = fp.advance_segments(frame, factor, decode, **want)
            assert (getattr(one, name) == getattr(full, name)).all(), (name, factor)
            assert all(getattr(one, n) is None for n in ("klass", "conf", "stats", "rgba") if n != name)
            uone = run(ctx, outs[0], decode, **want)
            assert (getattr(uone, name) == getattr(ufull, name)).all(), name


# --------------------------------------------------------------------------- #
# 6. graph replay
# --------------------------------------------------------------------------- #
def test_segments_calls_leave_the_cached_graphs_alone(blob50):
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
            s = fg.advance_segments(fr, 1.0, SOFTMAX if it & 1 else RAW, want_rgba=True)
            e = fe.advance_segments(fr, 1.0, SOFTMAX if it & 1 else RAW, want_rgba=True)
            assert all((x == y).all() for x, y in zip(s[:4], e[:4]))
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
            if not it & 1:
                assert (s.rgba == b).all()
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a segments call caused a capture"
        assert cached1 >= cached0, "a segments call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the segments calls were not replayed"
