"""The fused decode -- FramePath.advance_segments in both decodes with all four outputs, FramePath.advance's mask, Model.advance's
planar output -- at every class count, head form and edge size (tests/heads.py has the table; tests/test_decode_heads_cpu.py proves
that it reaches every form and that the crafted heads are not vacuous).  Everything is graded given the run's own low-res logits:
``oracle.upsample_bilinear(model.lowres())`` -> ``segments_ref.decode`` / ``stats`` and ``oracle.colorcode``.  No tolerances: the
planar output, the mask, the RAW decode and the SOFTMAX class plane are compared with ``==``; the SOFTMAX confidence by the rules of
test_unfused_softmax (exact outside ``segments_ref.in_band``, within 1 inside it, at most 1 % of a case's pixels in the band).

What runs (f32 mode, FCN-ResNet50 on the synthetic parameters, frame index = K):

  float heads    K = 1 2 3 4 | 5 8 | 11 | 14 | 17 20 | 23 24 -> upsample_argmax_segments_lds_kernel<1> .. <6> with 3, 2, 1 and 0 pad
                 classes at more than one NQ each; K = 25, 31 -> the scalar kernel; each at 52x100 (dword stores), 50x99 (byte stores),
                 17x65 (one live pixel in the second tile row / column), 9x9, 4x1 and 1x3 (staged, every tile coordinate clamped) and
                 3x1, 1x2, 2x1, 1x1 (scalar: the staged footprint exceeds 48 KB); 64 guard bytes behind every output at 50x99, 17x65
  crafted heads  K = 5, 22, 23 (<2>, <6>, <6>; 3, 2, 1 pad classes), 26 (scalar) at 52x100, 50x99, 17x65, 1x3, 1x2 with classifier.4
                 rewritten: every logit negative (a zero pad class would win RAW-style and add exp(-max) to the softmax sum); twin
                 classes (exact ties: the first maximum wins); +inf / NaN / -inf biases (0 * inf = NaN on the border)
  quantised      K = 6, 21, 26 (<2>, <6>, scalar) at 52x100, 50x99, 1x2 on models that resize the u8 codes of their heads before
                 DequantizeLinear (up_post; exact top-2 ties on 1-4 % of the pixels)

In-band shares, all sizes of a case pooled: float heads 0.26-0.51 % for K >= 2 (K = 1: p = 1, conf 255, every pixel on an integer:
exempt), crafted heads 0.02-0.49 % (the non-finite heads 0.02-0.12 %: +inf owns the interior), quantised heads 0.28-0.36 % on the
GPU's own logits; the float64 / integer references of test_decode_heads_cpu.py give the same within 0.1 %.  Each case prints its share.

With the pad fix-up of the staged kernel changed from -inf to 0.f (a scratch build) every staged case with K % 4 != 0 fails: the
all-negative heads at K = 5, 22, 23 because a pad class wins, the others on the SOFTMAX confidence or a class index >= K.

Measured on an MI355X: 14 s from the first case to the last for the 29 cases, 0.3-0.9 s each (2.3 s for the first, which makes the
shared tensors).
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd.processors import Context, FramePath, Model, ModelCmd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads as H  # noqa: E402
import segments_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX


@pytest.fixture(scope="module", autouse=True)
def module_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_decode_heads.py: {time.perf_counter() - t0:.0f} s from the first case to the last")


class Run:
    """what one frame left: both decodes, the mask, the planar outputs and the low-res logits they were all made from"""

    def __init__(self, ctx, model, frame, what):
        fp = FramePath(ctx)
        self.raw = fp.advance_segments(frame, 1.0, RAW, want_rgba=True)
        self.lo, self.aux = model.lowres()
        self.sm = fp.advance_segments(frame, 1.0, SOFTMAX, want_rgba=True)
        self.mask, _ = fp.advance(frame, 1.0)
        self.planar = []
        model.advance(frame, self.planar)
        # the conv stack is deterministic: all four calls decoded the same logits
        lo2, _ = model.lowres()
        assert (self.lo.view(np.uint32) == lo2.view(np.uint32)).all(), what


def compare(ref, run, lut, what, planar_ref=None, nan_planar=False):
    """one frame against its reference -> (pixels in the band, pixels)"""
    H.check_raw(ref, run.raw, what + " RAW")
    H.check_softmax(ref, run.sm, lut, what + " SOFTMAX")
    assert (run.mask == ref.mask).all(), (what, "advance mask")
    for got, want in zip(run.planar, planar_ref if planar_ref is not None else [ref.up]):
        if nan_planar:
            assert H.same_floats(got, want), (what, "planar")
        else:
            assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all(), (what, "planar")
    return int(ref.band.sum()), ref.band.size


def band_cap(what, band, pixels, exempt=False):
    print(f"{what}: {band} of {pixels} pixels in the band ({100.0 * band / pixels:.2f} %)")
    assert exempt or band <= H.BAND_CAP * pixels, (what, band, pixels)


def guard_bytes(ctx, K, frame, run, what):
    """infur_frame_segments_dev into poisoned device buffers: the outputs are the host path's, the 64 bytes behind each survive"""
    L, h = ctx.L, ctx.h
    hh, ww = frame.shape[:2]
    hw = hh * ww
    sizes = {"klass": hw, "conf": hw, "stats": K * 64, "rgba": hw * 4}
    dev = {}
    try:
        for name, n in list(sizes.items()) + [("bgr", frame.nbytes)]:
            d = C.c_void_p(None)
            ctx.check(L.infur_dev_alloc(h, n + 64, C.byref(d)))
            dev[name] = d
        ctx.check(L.infur_memcpy_h2d(h, dev["bgr"], frame.ctypes.data, frame.nbytes))
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        for mode, s in ((RAW, run.raw), (SOFTMAX, run.sm)):
            for name, n in sizes.items():
                poison = np.full(n + 64, 0xA5, np.uint8)
                ctx.check(L.infur_memcpy_h2d(h, dev[name], poison.ctypes.data, n + 64))
            ctx.check(L.infur_frame_segments_dev(h, dev["bgr"], ww, hh, 1.0, 0, mode, dev["klass"], dev["conf"], hw, dev["stats"], K, dev["rgba"],
                                                 hw * 4, None, C.byref(ow), C.byref(oh)))
            ctx.synchronize()
            got = {}
            for name, n in sizes.items():
                b = np.empty(n + 64, np.uint8)
                ctx.check(L.infur_memcpy_d2h(h, b.ctypes.data, dev[name], n + 64))
                assert (b[n:] == 0xA5).all(), (what, name, mode)
                got[name] = b[:n]
            assert (got["klass"] == s.klass.ravel()).all() and (got["conf"] == s.conf.ravel()).all(), (what, mode)
            assert (got["stats"].view(np.uint64).reshape(K, 8) == s.stats).all() and (got["rgba"] == s.rgba.ravel()).all(), (what, mode)
    finally:
        for d in dev.values():
            ctx.check(L.infur_dev_free(h, d))


# ---- 2. class counts and sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", H.FLOAT_KS)
def test_every_class_count_at_every_size(oracle, tables, K):
    lut = tables["color_lut"]
    band = pixels = 0
    with Context(device=0) as c:
        m = Model(c).control(ModelCmd.LoadBlob(H.float_blob(K)))
        info = m.get_info()
        assert info.num_classes == K and info.output_names == ["out"]
        for size in H.SIZES:
            what = f"K {K} {size[0]}x{size[1]} form {H.form_of(K, size)}"
            frame = H.frame(K, size)
            run = Run(c, m, frame, what)
            assert run.lo.shape[0] == K and np.isfinite(run.lo).all(), what
            ref = H.Ref(oracle.upsample_bilinear(run.lo, size[0], size[1]), oracle)
            b, p = compare(ref, run, lut, what)
            band, pixels = band + b, pixels + p
            if size in H.GUARD_SIZES:
                guard_bytes(c, K, frame, run, what)
    band_cap(f"float head K {K}", band, pixels, exempt=K == 1)


# ---- 3. crafted heads ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", H.CRAFTED_KS)
@pytest.mark.parametrize("head", H.CRAFTED_HEADS)
def test_crafted_heads(oracle, tables, head, K):
    lut = tables["color_lut"]
    band = pixels = 0
    pairs = H.twin_pairs(K)
    later = [j for _, j in pairs]
    with Context(device=0) as c:
        m = Model(c).control(ModelCmd.LoadBlob(H.crafted_blob(head, K)))
        assert m.get_info().num_classes == K
        for size in H.CRAFTED_SIZES:
            what = f"{head} K {K} {size[0]}x{size[1]} form {H.form_of(K, size)}"
            run = Run(c, m, H.frame(K, size), what)
            ref = H.Ref(oracle.upsample_bilinear(run.lo, size[0], size[1]), oracle)
            if head == "negative":
                assert (ref.up < 0).all(), what  # (the conv stack's f32 logits, like the float64 ones of the CPU test)
                s = run.raw
                assert (s.klass == 0).all() and (s.conf == 0).all() and s.stats[0, R.PIXELS] == s.klass.size and (s.stats[1:, R.PIXELS] == 0).all(), what
                assert (run.sm.klass == ref.up.argmax(axis=0)).all(), what
            elif head == "twins":
                for i, j in pairs:  # a finding about the conv kernels if not: two output channels with the same weights
                    assert (run.lo[i].view(np.uint32) == run.lo[j].view(np.uint32)).all(), (what, i, j)
                assert not np.isin(run.raw.klass, later).any() and not np.isin(run.sm.klass, later).any(), what
                assert (run.raw.stats[later, R.PIXELS] == 0).all() and (run.sm.stats[later, R.PIXELS] == 0).all(), what
            else:
                assert np.isnan(run.lo[1]).all() and (run.lo[2] == np.inf).all() and (run.lo[4] == -np.inf).all(), what
            b, p = compare(ref, run, lut, what, nan_planar=head == "nonfinite")
            band, pixels = band + b, pixels + p
    band_cap(f"{head} head K {K}", band, pixels)


# ---- 4. quantised heads that resize their codes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", H.QUANT_KS)
def test_quantised_heads_that_resize_their_codes(oracle, tables, K):
    lut = tables["color_lut"]
    band = pixels = 0
    _, blob_r = H.quant_blobs(K)
    with Context(device=0) as c:
        m = Model(c).control(ModelCmd.LoadBlob(blob_r))
        info = m.get_info()
        assert info.num_classes == K and info.quantised and info.resize_u8_heads
        for size in H.QUANT_SIZES:
            what = f"quantised K {K} {size[0]}x{size[1]} form {H.form_of(K, size)}"
            run = Run(c, m, H.frame(K, size), what)
            ups, lows = H.quant_reference_planes(K, size, oracle)
            # the run's own logits are the integer oracle's (read back dequantised): the codes are the run's own
            assert (run.lo.view(np.uint32) == lows[0].view(np.uint32)).all() and (run.aux.view(np.uint32) == lows[1].view(np.uint32)).all(), what
            ref = H.Ref(ups[0], oracle)
            b, p = compare(ref, run, lut, what, planar_ref=ups)
            assert len(run.planar) == 2, what
            band, pixels = band + b, pixels + p
    band_cap(f"quantised head K {K}", band, pixels)
