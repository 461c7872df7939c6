"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle.

Bit-exact for the byte/index stages (Scale, pre-proc, ColorCode, up-sample given the same
low-res logits, fused vs unfused); the conv stack is checked against the oracle within the
north-star tolerance of 1e-3 relative (f32), stated in REL_TOL below.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import (ColorCode, Context, Frame, FramePath, InfurError, Model, ModelCmd,
                                  ModelCmdError, Scale, ScaleProcError, Slot, ValidScaleError,
                                  bgr_image, pack_normalize)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402

pytestmark = pytest.mark.gpu

# The conv stack against an oracle is graded by tests/accuracy.py: four readings (max-abs / max-abs, worst per element, rms, bias), each
# at min(the bar below, 1.3 x measured).  REL_TOL and ELEM_TOL stay as the names of the old bars (the table's WAS entries): REL_TOL is also
# the width of the tie band of the class map.
REL_TOL = A.WAS[("f32", "friendly/logits")][0]  # 1e-3, north_star: "logits within 1e-3 relative fp32"


# max-abs / max-abs lets one large logit hide errors on the small ones, so the forward tests also grade the worst
# PER-ELEMENT relative error over the elements with |ref| > 1e-2 max |ref| (the metric of tests/hostile.py::errors).  Measured in
# the native f32 mode: 2e-4 (logits), 4e-4 (per layer), on friendly and hostile weights alike; the bar is 1e-3 like the other.
ELEM_TOL = A.WAS[("f32", "friendly/logits")][1]  # 1e-3

rel_err, elem_err = A.rel_err, A.elem_err  # (one definition: tests/accuracy.py::readings)


# --------------------------------------------------------------------------- #
# Scale (processing.rs:179-282)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("mode", [_lib.SCALE_NEAREST, _lib.SCALE_BILINEAR])
@pytest.mark.parametrize("wh", [(64, 48), (97, 61), (640, 480), (1280, 720), (1, 1), (3, 2), (1921, 1079)])
def test_scale_matches_oracle(ctx, oracle, mode, wh):
    w, h = wh
    fr = W.synth_frame(h, w, index=w)
    for fac in (0.5, 0.37, 0.999, 1.7, 2.0, 0.1):
        rc, ref = oracle.scale(fr, fac, mode)
        s = Scale(ctx, mode).control(fac)
        out = Slot()
        if rc != 0:
            with pytest.raises(ScaleProcError) as e:
                s.advance(Frame(1, fr), out)
            assert e.value.code == rc
            continue
        s.advance(Frame(7, fr), out)
        assert out.value.id == 7 and out.value.img.shape == ref.shape
        assert (out.value.img == ref).all(), (wh, fac, mode)


def test_scale_golden(ctx, golden):
    for tag in ("64x48", "97x61"):
        fr = golden[f"bgr_{tag}"]
        for mn, mode in (("nearest", 0), ("bilinear", 1)):
            for fac in (0.5, 0.37, 1.7):
                out = Slot()
                Scale(ctx, mode).control(fac).advance(Frame(0, fr), out)
                assert (out.value.img == golden[f"scale_{mn}_{fac}_{tag}"]).all()


def test_scale_reference_behaviour(ctx, kats):
    """processing.rs:289-303 and app.rs:187,199,216 through the HIP-backed Scale."""
    s = Scale(ctx)
    assert s.is_dirty()  # Default: dirty = true
    s.control(0.99)
    with pytest.raises(ScaleProcError) as e:
        s.advance(Frame(0, bgr_image(0, 10)), Slot())
    assert e.value.kind == "ZeroSizeIn"
    s.control(0.00000001)
    with pytest.raises(ScaleProcError) as e:
        s.advance(Frame(0, bgr_image(10, 10)), Slot())
    assert e.value.kind == "ZeroSizeOut"
    for f in kats["valid_scale_rejects"]["factors"]:
        with pytest.raises(ValidScaleError):
            s.control(f)
    assert s.factor == np.float32(0.00000001)  # failed control leaves state untouched
    for d in kats["scale_dims"]:
        out = Slot()
        Scale(ctx).control(d["factor"]).advance(Frame(3, W.synth_frame(d["h"], d["w"])), out)
        assert out.value.img.shape == (d["oh"], d["ow"], 3) and out.value.id == 3
    # dirty flag transitions (processing.rs:222,233)
    s = Scale(ctx).control(0.5)
    assert s.is_dirty()
    out = Slot()
    s.advance(Frame(1, bgr_image(8, 8)), out)
    assert not s.is_dirty()
    s.control(0.5)
    assert not s.is_dirty()
    s.control(0.25)
    assert s.is_dirty()
    s.advance(None, out)  # None input: only clears dirty
    assert not s.is_dirty() and out.value.img.shape == (4, 4, 3)
    # unit scale clones; buffer reuse on same size
    s = Scale(ctx)
    img = W.synth_frame(9, 11)
    out = Slot()
    s.advance(Frame(5, img), out)
    assert (out.value.img == img).all() and out.value.img is not img
    s.control(0.5)
    s.advance(Frame(6, img), out)
    buf = out.value.img
    s.advance(Frame(7, img), out)
    assert out.value.img is buf and out.value.id == 7


# --------------------------------------------------------------------------- #
# pre-proc (predict_onnx.rs:103-137)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("wh", [(64, 48), (97, 61), (1, 1), (5, 3), (640, 480), (1920, 1080)])
def test_pack_normalize_bit_exact(ctx, oracle, wh):
    w, h = wh
    fr = W.synth_frame(h, w, index=11)
    got = pack_normalize(ctx, fr)
    ref = oracle.pack_normalize(fr)
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def test_pack_normalize_all_bytes(ctx, tables):
    fr = np.zeros((16, 16, 3), np.uint8)
    fr[..., 0] = np.arange(256).reshape(16, 16)            # B
    fr[..., 1] = np.arange(256).reshape(16, 16)[::-1]      # G
    fr[..., 2] = np.arange(256).reshape(16, 16).T          # R
    got = pack_normalize(ctx, fr)
    lut = tables["preproc_lut"]
    assert (got[0] == lut[0][fr[..., 2]]).all() and (got[1] == lut[1][fr[..., 1]]).all() and (got[2] == lut[2][fr[..., 0]]).all()


# --------------------------------------------------------------------------- #
# device pointers need only the natural alignment of their element type (include/infur_hip.h): pack_normalize and bgr_to_rgba take
# their vector path (dword loads, 16-byte stores) only for 16-byte aligned pointers and whole quads of pixels, and the scalar path
# otherwise -- which freshly allocated (256-byte aligned) buffers never reach when npix % 4 == 0
# --------------------------------------------------------------------------- #
POISON = 0xA5


class GuardedDev:
    """a device buffer of `n` bytes at byte offset `off` inside a poisoned allocation, 64 guard bytes behind it"""

    def __init__(self, ctx, n, off, data=None):
        self.ctx, self.n, self.off, self.total = ctx, n, off, off + n + 64
        self.d = C.c_void_p(None)
        ctx.check(ctx.L.infur_dev_alloc(ctx.h, self.total, C.byref(self.d)))
        host = np.full(self.total, POISON, np.uint8)
        if data is not None:
            host[off:off + n] = np.ascontiguousarray(data).view(np.uint8).ravel()
        ctx.check(ctx.L.infur_memcpy_h2d(ctx.h, self.d, host.ctypes.data, self.total))
        self.ptr = C.c_void_p(self.d.value + off)

    def read(self, what):
        """the n bytes; the bytes before them and the guard behind them must still hold the poison"""
        host = np.empty(self.total, np.uint8)
        self.ctx.check(self.ctx.L.infur_memcpy_d2h(self.ctx.h, host.ctypes.data, self.d, self.total))
        assert (host[:self.off] == POISON).all() and (host[self.off + self.n:] == POISON).all(), ("written outside the buffer", what)
        return host[self.off:self.off + self.n].copy()

    def free(self):
        self.ctx.check(self.ctx.L.infur_dev_free(self.ctx.h, self.d))


@pytest.mark.parametrize("wh", [(8, 4), (5, 3), (1, 1)])  # npix % 4 == 0 (the vector path when aligned), ragged, one pixel
def test_pre_proc_and_display_at_unaligned_device_pointers(ctx, oracle, wh):
    w, h = wh
    fr = W.synth_frame(h, w, index=13)
    ref_chw = oracle.pack_normalize(fr)
    ref_rgba = np.concatenate([fr[..., ::-1], np.full((h, w, 1), 255, np.uint8)], axis=-1)  # app.rs:132-144: [r, g, b, 255]
    for in_off in (0, 1, 2, 3):
        d_in = GuardedDev(ctx, fr.nbytes, in_off, fr)
        for out_off in (0, 4, 8, 12):
            what = (wh, in_off, out_off)
            d_chw = GuardedDev(ctx, ref_chw.nbytes, out_off)
            ctx.check(ctx.L.infur_pack_normalize_dev(ctx.h, d_in.ptr, w, h, d_chw.ptr))
            ctx.synchronize()
            assert (d_chw.read(what).view(np.uint32) == ref_chw.view(np.uint32).ravel()).all(), what
            d_chw.free()
            d_rgba = GuardedDev(ctx, w * h * 4, out_off)
            ctx.check(ctx.L.infur_bgr_to_rgba_dev(ctx.h, d_in.ptr, w, h, d_rgba.ptr))
            ctx.synchronize()
            assert (d_rgba.read(what) == ref_rgba.ravel()).all(), what
            d_rgba.free()
        assert (d_in.read((wh, in_off)) == fr.ravel()).all()
        d_in.free()


def test_frame_advance_dev_at_unaligned_frame_pointers(ctx, model):
    """the stem reads the frame's bytes: a frame at byte offset 1, 2, 3 gives the aligned call's mask byte for byte"""
    w = h = 8
    fr = W.synth_frame(h, w, index=17)
    masks = []
    for in_off in (0, 1, 2, 3):
        d_in, d_rgba = GuardedDev(ctx, fr.nbytes, in_off, fr), GuardedDev(ctx, w * h * 4, 0)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        ctx.check(ctx.L.infur_frame_advance_dev(ctx.h, d_in.ptr, w, h, 1.0, 0, d_rgba.ptr, w * h * 4, None, C.byref(ow), C.byref(oh)))
        ctx.synchronize()
        assert (ow.value, oh.value) == (w, h)
        masks.append(d_rgba.read(in_off))
        assert (d_in.read(in_off) == fr.ravel()).all()
        d_in.free()
        d_rgba.free()
    ref, _ = FramePath(ctx).advance(fr, 1.0)
    assert all((m == ref.ravel()).all() for m in masks)


# --------------------------------------------------------------------------- #
# ColorCode (decode_predict.rs:32-79)
# --------------------------------------------------------------------------- #
def test_colorcode_reference_kats(ctx, oracle, kats):
    k = kats["decode_0to1"]
    hm = np.linspace(0.0, 1.0, k["linspace"][2], dtype=np.float32).reshape(k["shape"])
    out = Slot()
    ColorCode(ctx).advance(hm, out)
    img = out.value
    assert img.shape == (k["height"], k["width"], 4)
    conf = 0
    for p in img.reshape(-1, 4):
        assert (p == oracle.color_code(k["klass"], np.float32(p[3]) / np.float32(255.0))).all()
        assert conf <= p[3]
        conf = p[3]
    assert conf == k["last_alpha"]
    # color_2: a single pixel whose only positive class is 2 with confidence 0.5
    one = np.zeros((3, 1, 1), np.float32)
    one[2] = kats["color_2"]["alpha"]
    out = Slot()
    ColorCode(ctx).advance(one, out)
    r, g, b, a = kats["color_2"]["unmultiplied_rgba"]
    assert (out.value[0, 0] == oracle.from_rgba_unmultiplied(r, g, b, a)).all()


def test_colorcode_edge_cases_and_random(ctx, oracle, golden):
    out = Slot()
    cc = ColorCode(ctx)
    cc.advance(golden["cc_in"], out)
    assert (out.value == golden["cc_rgba"]).all()
    rng = np.random.default_rng(5)
    for k, h, w in ((21, 33, 47), (1, 4, 4), (22, 24, 32), (40, 7, 9), (21, 270, 480)):
        x = rng.normal(0.4, 0.5, size=(k, h, w)).astype(np.float32)
        x[rng.random(x.shape) < 0.01] = np.nan
        x[rng.random(x.shape) < 0.01] = np.inf
        x[rng.random(x.shape) < 0.01] = -np.inf
        cc.advance(x, out)
        assert out.value.shape == (h, w, 4)
        assert (out.value == oracle.colorcode(x)).all()
    # empty image and reuse on same size
    cc.advance(np.zeros((21, 0, 5), np.float32), out)
    assert out.value.shape == (0, 5, 4)


def test_color_lut_every_entry(ctx, tables):
    """All 20 x 256 (class, alpha) pairs through the kernel == the oracle's epaint table."""
    lut = tables["color_lut"]
    x = np.zeros((20, 20, 256), np.float32)
    for k in range(20):
        # pixel (k, a): class k has confidence with (c*255) as u8 == a
        x[k, k, :] = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0)
    x[:, :, 0] = 0.0
    out = Slot()
    ColorCode(ctx).advance(x, out)
    got = out.value
    exp_a = np.minimum((x.max(0) * np.float32(255.0)).astype(np.int64), 255)
    for k in range(20):
        assert (got[k] == lut[k, exp_a[k]]).all(), k


# --------------------------------------------------------------------------- #
# Model (predict_onnx.rs:283-345) -- conv stack within tolerance of the oracle
# --------------------------------------------------------------------------- #
def test_model_info_and_load_errors(ctx, model, blob50):
    info = model.get_info()
    assert info.input_names == ["input"] and info.output_names == ["out", "aux"] and info.input0_dtype == "Float"
    assert info.num_classes == 21 and info.depth == 50
    c2 = Context(device=0)
    m = Model(c2)
    assert m.get_info() is None
    out = ["sentinel"]
    m.advance(bgr_image(32, 24), out)  # no model: Ok(()) and `out` untouched (predict_onnx.rs:318,333)
    assert out == ["sentinel"]
    with pytest.raises(ModelCmdError) as e:
        m.control(ModelCmd.LoadBlob(b"NOTABLOB" + bytes(100)))
    assert e.value.code == _lib.E_MODEL_FORMAT
    with pytest.raises(ModelCmdError):
        m.control(ModelCmd.LoadBlob(blob50[:1000]))  # truncated
    bad = bytearray(blob50[: 32 + 57 * 80 + 64])
    with pytest.raises(ModelCmdError):
        m.control(ModelCmd.LoadBlob(bytes(bad)))  # table ok, data out of range
    with pytest.raises(ModelCmdError) as e:
        m.control(ModelCmd.Load("/nonexistent/model.bin"))
    assert e.value.code == _lib.E_IO
    assert m.get_info() is None
    m.control(ModelCmd.LoadBlob(blob50))
    assert m.get_info() is not None
    m.control(ModelCmd.Load(""))  # empty path unloads (predict_onnx.rs:310-312)
    assert m.get_info() is None
    rgba, scaled = FramePath(c2).advance(W.synth_frame(24, 32), 0.5, want_scaled=True)
    assert rgba is None and scaled.shape == (12, 16, 3)  # mask cleared, frame still scaled (app.rs:127-129)
    c2.close()


def test_model_load_from_file(ctx, blob50, tmp_path, oracle_model):
    p = tmp_path / "fcn.infurw"
    p.write_bytes(blob50)
    c2 = Context(device=0)
    m = Model(c2).control(ModelCmd.Load(str(p)))
    fr = W.synth_frame(48, 64)
    out = []
    m.advance(fr, out)
    lo, _ = m.lowres()
    ref = oracle_model.model_forward(oracle_model.pack_normalize(fr), full=False)
    assert A.grade(lo, ref["out_low"], "f32", "friendly/logits", "64x48 out, loaded from a file")[0] < REL_TOL
    c2.close()


@pytest.mark.parametrize("tag", ["64x48", "97x61"])
def test_model_against_golden(ctx, model, golden, oracle, tag):
    fr = golden[f"bgr_{tag}"]
    out = []
    model.advance(fr, out)
    assert len(out) == 2
    lo, la = model.lowres()
    for got, key in ((lo, "out_low"), (la, "aux_low"), (out[0], "out"), (out[1], "aux")):
        assert A.grade(got, golden[f"{key}_{tag}"], "f32", "friendly/logits", f"golden {tag} {key}")[0] < REL_TOL
    # the up-sample kernel itself is bit-exact given the same low-res logits
    h, w = fr.shape[:2]
    assert (out[0].view(np.uint32) == oracle.upsample_bilinear(lo, h, w).view(np.uint32)).all()
    assert (out[1].view(np.uint32) == oracle.upsample_bilinear(la, h, w).view(np.uint32)).all()


def test_model_per_layer_against_torch_oracle(blob50):
    """Every conv output (keep_activations) against the torch-CPU restatement."""
    from oracle.infur_oracle import COracle, TorchModel

    co = COracle()
    tm = TorchModel(blob50)
    c2 = Context(device=0, keep_activations=True)
    m = Model(c2).control(ModelCmd.LoadBlob(blob50))
    fr = W.synth_frame(72, 104, index=2)
    out = []
    m.advance(fr, out)
    taps = {}
    tm.forward_lowres(co.pack_normalize(fr), taps=taps)
    worst = worst_e = 0.0
    for i, spec in enumerate(W.graph(50)):
        ref = taps[spec.name].numpy()
        buf = np.empty(ref.shape, np.float32)
        c, h, w = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        c2.check(c2.L.infur_debug_read_activation(c2.h, i, buf.ctypes.data, buf.size, C.byref(c), C.byref(h), C.byref(w)))
        assert (c.value, h.value, w.value) == ref.shape, spec.name
        e, ee = A.grade(buf, ref, "f32", "friendly/layer", f"104x72 {spec.name}", cap=(None, ELEM_TOL, None, None))[:2]
        worst, worst_e = max(worst, e), max(worst_e, ee)
        assert e < REL_TOL and ee < ELEM_TOL, (spec.name, e, ee)
    print(f"worst per-layer error: max-abs / max-abs {worst:.2e}, per element {worst_e:.2e}")
    c2.close()


def test_infer_seg_model_shape(ctx, model, kats):
    """predict_onnx.rs:371-381: black 320x240 frame -> 2 tensors of shape [21,240,320]."""
    k = kats["infer_seg_model"]
    out = []
    model.advance(bgr_image(k["w"], k["h"]), out)
    assert len(out) == k["n_outputs"]
    assert list(out[0].shape) == k["shape"] and list(out[1].shape) == k["shape"]
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()


# --------------------------------------------------------------------------- #
# fused frame path (app.rs:107-153)
# --------------------------------------------------------------------------- #
def argmax_report(oracle, got_rgba, ref_logits, tol_logits):
    """Mismatching pixels are acceptable only where the oracle's top-2 gap is inside the logit tolerance."""
    ref_rgba = oracle.colorcode(ref_logits)
    bad = (got_rgba != ref_rgba).any(-1)
    if not bad.any():
        return 0, 0.0
    srt = np.sort(np.maximum(ref_logits, 0.0), axis=0)
    gap = srt[-1] - srt[-2]
    # alpha may also differ by one step where c_max*255 sits on an integer boundary
    kl, al = oracle.argmax(ref_logits)
    frac = ref_logits.max(0) * 255.0
    near_alpha = np.abs(frac - np.round(frac)) < tol_logits * 255.0
    unexplained = bad & ~((gap < tol_logits) | near_alpha)
    return int(bad.sum()), float(unexplained.mean())


@pytest.mark.parametrize("tag", ["64x48", "97x61"])
def test_frame_advance_small(ctx, model, golden, oracle, tag):
    fr = golden[f"bgr_{tag}"]
    fp = FramePath(ctx)
    rgba, _ = fp.advance(fr, 1.0)
    lo, _ = model.lowres()
    h, w = fr.shape[:2]
    # fused kernel == oracle up-sample + ColorCode on the same low-res logits, bit for bit
    assert (rgba == oracle.colorcode(oracle.upsample_bilinear(lo, h, w))).all()
    # against the whole-path oracle: class map identical except at near-ties
    nbad, unexplained = argmax_report(oracle, rgba, golden[f"out_{tag}"], REL_TOL * np.abs(golden[f"out_{tag}"]).max())
    assert unexplained == 0.0, (nbad, unexplained)
    assert nbad <= 0.01 * h * w


def test_frame_advance_scaled_equals_unfused(ctx, model, oracle):
    """scale -> model -> decode fused == Scale, Model, ColorCode processors chained (app.rs:107-123)."""
    fr = W.synth_frame(180, 320, index=4)
    for mode in (0, 1):
        rgba, scaled = FramePath(ctx, mode).advance(fr, 0.5, want_scaled=True)
        s_out = Slot()
        Scale(ctx, mode).control(0.5).advance(Frame(0, fr), s_out)
        assert (scaled == s_out.value.img).all()
        m_out = []
        model.advance(s_out.value.img, m_out)
        c_out = Slot()
        ColorCode(ctx).advance(m_out[0], c_out)
        assert (rgba == c_out.value).all()


@pytest.mark.parametrize("wh", [(1920, 1080), (960, 540), (640, 480)])
def test_full_size_properties(ctx, model, oracle, blob50, wh):
    """BASELINE configs C2/C3 at full size and configs[0]'s 640x480 clip frame: determinism, fused == unfused, logits vs
    the torch-CPU oracle."""
    from oracle.infur_oracle import TorchModel

    w, h = wh
    fr = W.synth_frame(h, w, index=1)
    fp = FramePath(ctx)
    rgba1, _ = fp.advance(fr, 1.0)
    rgba2, _ = fp.advance(fr, 1.0)
    assert (rgba1 == rgba2).all()  # deterministic
    lo, la = model.lowres()
    assert (rgba1 == oracle.colorcode(oracle.upsample_bilinear(lo, h, w))).all()
    tl, ta = TorchModel(blob50).forward_lowres(oracle.pack_normalize(fr))
    e_out, p_out, s_out, b_out = A.grade(lo, tl.numpy(), "f32", "friendly/logits", f"{w}x{h} out")
    e_aux, p_aux, s_aux, b_aux = A.grade(la, ta.numpy(), "f32", "friendly/logits", f"{w}x{h} aux")
    print(f"{w}x{h}: low-res logits max-abs / max-abs out={e_out:.2e} aux={e_aux:.2e}; worst per-element out={p_out:.2e} aux={p_aux:.2e}; "
          f"rms out={s_out:.2e} aux={s_aux:.2e}; bias out={b_out:.2e} aux={b_aux:.2e}")
    assert e_out < REL_TOL and e_aux < REL_TOL
    assert p_out < ELEM_TOL and p_aux < ELEM_TOL
    ref_full = oracle.upsample_bilinear(tl.numpy(), h, w)
    nbad, unexplained = argmax_report(oracle, rgba1, ref_full, REL_TOL * np.abs(ref_full).max())
    print(f"{w}x{h}: {nbad} of {h*w} mask pixels differ from the CPU path; unexplained fraction {unexplained}")
    assert unexplained == 0.0 and nbad <= 0.005 * h * w
    assert (rgba1[..., 3] > 0).any()


def test_profile_records(blob50):
    c2 = Context(device=0, profile=True)
    Model(c2).control(ModelCmd.LoadBlob(blob50))
    rgba, _ = FramePath(c2).advance(W.synth_frame(96, 128), 1.0)
    recs = c2.profile()
    names = [r["name"] for r in recs]
    # 57 convs in 53 launches (conv3 and the downsample branch of each stage's first block are one two-source
    # GEMM) + maxpool + fused post; the 14 stride-1 3x3 convs with Cin >= 128 (layer2 x3, layer3 x6, layer4 x3, both
    # heads) run in the Winograd domain and add an input and an output transform each
    wino = [r for r in recs if r["kernel"] in ("wino_input", "wino_output")]
    # (the stem convolution and the max-pool are one kernel)
    assert names[0] == "backbone.conv1+maxpool" and names[-1] == "out.resize+colorcode"
    assert sum(n.endswith("conv3+downsample") for n in names) == 4
    assert len(wino) == 28 and len(recs) == 53 + 1 + len(wino)
    algo = sum(r["algo_flops"] for r in recs)
    assert abs(algo - W.conv_flops(96, 128)["total"]) < 1e-6 * algo
    assert sum(r["flops"] for r in recs) < algo  # Winograd executes 2.25x - 4x fewer MACs on those layers
    assert all(r["ms"] > 0 for r in recs)
    c2.close()


def test_device_resident_entry_points(ctx, model, oracle):
    """_dev forms with caller-owned device buffers (torch used only as the allocator)."""
    import torch

    fr = W.synth_frame(120, 160, index=9)
    d_in = torch.from_numpy(fr).cuda()
    d_rgba = torch.empty((60, 80, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ow, oh = FramePath(ctx).advance_dev(d_in.data_ptr(), 160, 120, 0.5, d_rgba.data_ptr(), d_rgba.numel())
    ctx.synchronize()
    assert (ow, oh) == (80, 60)
    ref, _ = FramePath(ctx).advance(fr, 0.5)
    assert (d_rgba.cpu().numpy() == ref).all()
    with pytest.raises(InfurError) as e:
        FramePath(ctx).advance_dev(d_in.data_ptr(), 160, 120, 0.5, d_rgba.data_ptr(), 100)
    assert e.value.code == _lib.E_CAPACITY


def test_model_load_from_onnx_file(blob50, tmp_path, oracle_model):
    """ModelCmd::Load("*.onnx"): logits identical to loading the same weights as a blob, and the
    file's own tensor names are reported (predict_onnx.rs:89-92, "input -> out,aux")."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import onnx_writer as OW

    _, tensors = W.unpack_blob(blob50)
    model_bytes, _ = OW.fcn_model(tensors, W.graph(50))
    p = tmp_path / "fcn-resnet50-12.onnx"
    p.write_bytes(model_bytes)
    c2 = Context(device=0)
    m = Model(c2).control(ModelCmd.Load(str(p)))
    info = m.get_info()
    assert info.input_names == ["input"] and info.output_names == ["out", "aux"] and info.depth == 50
    fr = W.synth_frame(48, 64)
    out = []
    m.advance(fr, out)
    lo, la = m.lowres()
    m.control(ModelCmd.LoadBlob(blob50))
    m.advance(fr, out)
    lo2, la2 = m.lowres()
    assert (lo.view(np.uint32) == lo2.view(np.uint32)).all() and (la.view(np.uint32) == la2.view(np.uint32)).all()
    # a file that is neither: float tensors under quantised operators (a well-formed QOperator file loads: test_gpu_quant.py)
    for op, msg in (("QLinearConv", "QuantizeLinear"), ("ConvInteger", "dynamically quantised")):
        bad = tmp_path / "int8.onnx"
        bad.write_bytes(OW.fcn_model(tensors, W.graph(50), conv_op=op)[0])
        with pytest.raises(ModelCmdError) as e:
            m.control(ModelCmd.Load(str(bad)))
        assert e.value.code == _lib.E_MODEL_FORMAT and msg in str(e.value)
    c2.close()


@pytest.mark.parametrize("tile,min_cin", [(2, 64), (4, 64), (6, 64), (4, 0xFFFFFFFF)])
def test_winograd_variants_per_layer(blob50, tile, min_cin):
    """Every conv output with Winograd F(2x2) / F(4x4) / F(6x6) forced onto ALL stride-1 3x3 convs (dilation 1, 2
    and 4, ragged tile edges), and with Winograd disabled, against the torch-CPU restatement."""
    from oracle.infur_oracle import COracle, TorchModel

    co = COracle()
    tm = TorchModel(blob50)
    c2 = Context(device=0, keep_activations=True, winograd_min_cin=min_cin, winograd_tile=tile)
    m = Model(c2).control(ModelCmd.LoadBlob(blob50))
    fr = W.synth_frame(75, 109, index=6)  # odd size: sub-grids of unequal extent, partial tiles
    out = []
    m.advance(fr, out)
    taps = {}
    tm.forward_lowres(co.pack_normalize(fr), taps=taps)
    worst = 0.0
    for i, spec in enumerate(W.graph(50)):
        ref = taps[spec.name].numpy()
        buf = np.empty(ref.shape, np.float32)
        c, h, w = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        c2.check(c2.L.infur_debug_read_activation(c2.h, i, buf.ctypes.data, buf.size, C.byref(c), C.byref(h), C.byref(w)))
        e = A.grade(buf, ref, "f32", "friendly/layer", f"109x75 F({tile}x{tile}) min_cin {min_cin} {spec.name}")[0]
        worst = max(worst, e)
        assert e < REL_TOL, (spec.name, e)
    print(f"winograd tile {tile} min_cin {min_cin}: worst per-layer rel err {worst:.2e}")
    c2.close()


@pytest.mark.parametrize("wh", [(1, 1), (7, 5), (33, 17), (8, 8), (130, 66)])
def test_tiny_and_ragged_frames(ctx, model, oracle_model, wh):
    """Degenerate sizes: 1-pixel feature maps, ragged GEMM tiles, partial Winograd tiles."""
    w, h = wh
    fr = W.synth_frame(h, w, index=w + h)
    rgba, _ = FramePath(ctx).advance(fr, 1.0)
    lo, la = model.lowres()
    ref = oracle_model.model_forward(oracle_model.pack_normalize(fr), full=False)
    assert lo.shape == ref["out_low"].shape
    e_out = A.grade(lo, ref["out_low"], "f32", "edge", f"{w}x{h} out")[0]
    e_aux = A.grade(la, ref["aux_low"], "f32", "edge", f"{w}x{h} aux")[0]
    assert e_out < REL_TOL and e_aux < REL_TOL
    assert (rgba == oracle_model.colorcode(oracle_model.upsample_bilinear(lo, h, w))).all()
    out = []
    model.advance(fr, out)
    assert out[0].shape == (21, h, w)
    assert (out[0].view(np.uint32) == oracle_model.upsample_bilinear(lo, h, w).view(np.uint32)).all()


@pytest.mark.parametrize("dtype", ["f32", "f16", "f32s"])
def test_fused_stem_pool_matches_the_two_kernel_form(blob50, dtype):
    """stem 7x7/2 + max-pool 3x3/2 as one kernel (the 132.7 MB stem tensor is never written) against the two-kernel form
    at sizes that exercise ragged pooled tiles, odd stem extents and 1-pixel maps.  In the f32 mode both use the exact
    f32 MFMA with the same k order: bit-identical.  In the f16-rate modes the fused stem runs on the f16 matrix cores
    (f16 operands / f16 hi+lo pairs) while the two-kernel debug form stays exact f32: the logits agree within the
    mode's own tolerance."""
    lows = {}
    sizes = [(64, 48), (97, 61), (5, 3), (1, 1), (130, 66), (320, 240), (175, 93)]
    for fuse in (True, False):
        with Context(device=0, dtype=dtype, fuse_stem_pool=fuse) as c:
            m = Model(c).control(ModelCmd.LoadBlob(blob50))
            res = []
            for (w, h) in sizes:
                out = []
                m.advance(W.synth_frame(h, w, index=w), out)
                res.append([x.copy() for x in m.lowres()])
            lows[fuse] = res
    tol = {"f32": 0.0, "f16": 5e-3, "f32s": 2e-5}[dtype]
    for (w, h), a, b in zip(sizes, lows[True], lows[False]):
        for x, y in zip(a, b):
            if tol == 0.0:
                assert (x.view(np.uint32) == y.view(np.uint32)).all(), (dtype, w, h)
            else:
                e = rel_err(x, y)
                assert e < tol, (dtype, w, h, e)


@pytest.mark.parametrize("ncls", [1, 3, 4, 7, 12, 13, 17, 20, 24, 25, 31])
def test_post_kernels_for_other_class_counts(oracle, ncls):
    """The LDS-staged up-sample kernels are instantiated per ceil(K / 4) class quads and evaluate whole quads (the
    pad classes of a staged pixel are zeros); K > 24 takes the scalar fallback.  Every instantiation, at a ragged
    size: fused up-sample + argmax + shade == oracle up-sample -> ColorCode on the same low-res logits, and the
    planar up-sample of Model::advance == the oracle's, bit for bit."""
    blob = W.synth_blob(num_classes=ncls, aux=False)
    c = Context(device=0)
    m = Model(c).control(ModelCmd.LoadBlob(blob))
    assert m.get_info().num_classes == ncls
    fr = W.synth_frame(70, 131, index=ncls)
    h, w = fr.shape[:2]
    rgba, _ = FramePath(c).advance(fr, 1.0)
    lo, _ = m.lowres()
    up = oracle.upsample_bilinear(lo, h, w)
    assert (rgba == oracle.colorcode(up)).all()
    out = []
    m.advance(fr, out)
    lo2, _ = m.lowres()
    assert (lo2 == lo).all()
    assert out[0].shape == (ncls, h, w) and (out[0] == up).all()
    c.close()
