"""the numerics the headline depends on, on UNFRIENDLY data.  Every other suite uses one benign weight
distribution (uniform U(-a, a), BN gamma in [0.5, 1.5]); pretrained BN-folded weights have heavy tails and per-channel scales
orders of magnitude apart, and the default f32 path runs 14 convs as Winograd F(6x6, 3x3), whose error grows with the dynamic
range of weights and activations.  tests/hostile.py builds such a parameter set (1 % outliers at 30 sigma, per-channel scales
over 3.2 decades as an exact reparametrisation, always-on channels) and a frame with saturated regions; the HIP modes f32
(F(6x6) default), f32s, f32x (F(4x4) default) and -- for the record -- the reduced-precision f16 mode are graded per layer at 320x240 and on the whole 1920x1080 frame against a FLOAT64 evaluation of
the network (torch CPU), with two metrics: max-abs error / max-abs reference (the reading tests/test_gpu_parity.py uses)
and the worst per-element relative error over the elements with |ref| > 1e-2 max |ref|.  north_star's bar: logits within 1e-3."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import hostile as H  # noqa: E402

from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd

pytestmark = pytest.mark.gpu

# Measured on an MI355X (scripts/hostile_probe.py prints every mode x Winograd tile; profiles/r04_hostile_probe.log):
#   mode   logits 1080p (max-abs/max-abs | per-element)   per-layer worst
#   f32    3.8e-06 | 2.1e-04                               8.3e-06      exact f32 MFMA, F(6x6): as good as direct convs (4.1e-06)
#   f32s   1.6e-05 | 1.0e-03                               2.6e-05      F(6x6); direct convs 9.4e-06.  BEFORE round 3's per-plane
#                                                                      weight scales: 8.9e-03 .. 1.6e-02 -- outside the bar, found by this test
#   f32x   1.4e-04 | 1.0e-02                               3.9e-04      round 4: bf8 (e5m2) cross terms, F(6x6) (F(4x4): 1.1e-04 | 7.0e-03;
#                                                                      direct 1.0e-04 | 8.2e-03: the product error itself sits at the 1e-2
#                                                                      line).  Round 3's e4m3 cross terms under static scales: 7.1e-04 |
#                                                                      5.1e-02 -- heavy tails clamp and flush e4m3
#   f16    1.9e-03 | 1.3e-01                               4.5e-03      for the record: the reduced-precision mode (configs[4]'s arithmetic)
#                                                                      is OUTSIDE north_star's 1e-3; its own stated bar is 5e-3
# The logits bar is north_star's 1e-3 for every f32-grade mode.  VERDICT r3 asked for <= 1e-2 per element from a mode at f16-MFMA
# rate: f32s has it with 10x room; f32x sits AT it (7e-3 .. 1.03e-2 depending on the Winograd tile -- test_f32x_tiles below holds
# F(4x4) to 1e-2 and the F(6x6) default to 1.5e-2, and says so).  Per-layer bars: the measured values with ~3x head-room.
#   f16hl  1.5e-04 | 9.6e-03 (F(6x6) default; F(4x4) 1.2e-04 | 9.5e-03; per-layer path, direct convs 1.1e-04 | 8.2e-03)
#                                                          5.1e-04      round 5: three-byte tensors (f16 hi + e5m2 lo planes), two MFMA units per
#                                                                      product, every operand staged by LDS-DMA: VERDICT r4's bars -- logits 1e-3
#                                                                      AND 1e-2 per element on this set -- at 1.2x the f32x rate.  The per-element
#                                                                      figure is the format's: the simulation with EXACT products on three-byte
#                                                                      tensors reads 4.6e-3 at 320x240 (scripts/sim_hl_assign.py), this mode 6.7e-3
# The bars are tests/accuracy.py's: min(the bars above's history, 1.3 x measured) for each of FOUR readings (max-abs/max-abs, worst per
# element, rms, bias).  The names below stay as aliases of that table's values: LOGIT_BAR is also the width of the tie band of the class map.
MODES = ("f32", "f32s", "f32x", "f16", "f16hl")
LOGIT_BAR = {"f32": 1e-3, "f32s": 1e-3, "f32x": 1e-3, "f16": 5e-3, "f16hl": 1e-3}  # north_star's 1e-3 (f16: its own 5e-3): the tie band
LAYER_BAR = {m: A.WAS[(m, "hostile/layer")][0] for m in MODES}
LAYER_ELEM_BAR = {m: A.WAS[(m, "hostile/layer")][1] for m in MODES}
ELEM_BAR = {m: A.WAS[(m, "hostile/logits1080")][1] for m in MODES}
# Round 6: the same two figures as a DISTRIBUTION -- six hostile parameter sets (tests/hostile.py::SEEDS: other outlier
# positions / channel scales, three of them on other base tensors) x two frames at 960x540, profiles/r06_hostile_seeds_960x540.log:
#   f16hl   max-abs/max-abs 1.40e-4 .. 2.16e-4      per element 7.8e-3 .. 1.53e-2   (5 of 12 cases above 1e-2)
#   f32x                    1.29e-4 .. 1.88e-4                  7.5e-3 .. 1.65e-2
#   f32s                    1.38e-5 .. 2.26e-5                  8.1e-4 .. 1.07e-3
#   simulation, exact products on three-byte tensors (the FORMAT's floor)   6.0e-5 .. 7.8e-5 ; 3.5e-3 .. 5.1e-3
#   simulation, the kernel's products (both hi bytes truncated, debiased)    1.2e-4 .. 1.5e-4 ; 7.0e-3 .. 1.19e-2
# north_star's "logits within 1e-3" (max-abs reading) holds for f16hl on every set with >= 4.6x room.  The per-element 1e-2 that
# VERDICT r3/r4 asked for does NOT hold as a distribution: the metric's worst element sits at 1 % of the largest logit, where an
# absolute error of 1.5-2.2e-4 of the maximum IS 1.5-2.2e-2 relative; the one set of round 5 (9.6e-3) was a lucky sample.
SEED_MODES = ("f32", "f32s", "f32x", "f16hl")  # (f32 and f32s joined the sweep with the table: the float64 references are shared)
SEED_LOGIT_BAR = {m: A.WAS[(m, "hostile/seeds")][0] for m in SEED_MODES}
SEED_ELEM_BAR = {m: A.WAS[(m, "hostile/seeds")][1] for m in SEED_MODES}


@pytest.fixture(scope="module")
def hostile_blob():
    return H.hostile_blob()


@pytest.fixture(scope="module")
def ref64(hostile_blob):
    from oracle.infur_oracle import TorchModel

    return TorchModel(hostile_blob, float64=True)


@pytest.fixture(scope="module")
def ref1080(ref64, oracle):
    """the float64 logits of the historical set's 1920x1080 frame: made once, shared by the two tests that grade against them"""
    fr = H.saturated_frame(1080, 1920, index=2)
    ref, ref_aux = ref64.forward_lowres(oracle.pack_normalize(fr))
    return fr, ref.numpy(), ref_aux.numpy()


@pytest.mark.parametrize("dtype", ["f32", "f32s", "f32x", "f16", "f16hl"])
def test_per_layer_on_hostile_parameters(hostile_blob, ref64, oracle, dtype):
    fr = H.saturated_frame(240, 320)
    taps = {}
    ref64.forward_lowres(oracle.pack_normalize(fr), taps=taps)
    c = Context(device=0, dtype=dtype, keep_activations=True)
    m = Model(c).control(ModelCmd.LoadBlob(hostile_blob))
    out = []
    m.advance(fr, out)
    worst = (0.0, 0.0, "", "")
    table = []  # every layer's four readings: a layer whose rms or bias stands out from its neighbours is a defect (printed with -s)
    for i, spec in enumerate(W.graph(50)):
        ref = taps[spec.name].numpy()
        buf = np.empty(ref.shape, np.float32)
        cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        c.check(c.L.infur_debug_read_activation(c.h, i, buf.ctypes.data, buf.size, C.byref(cc), C.byref(hh), C.byref(ww)))
        e_max, e_rel, e_rms, e_bias = A.grade(buf, ref, dtype, "hostile/layer", f"320x240 {spec.name}")
        table.append(f"   {spec.name:34s} {e_max:.2e} {e_rel:.2e} {e_rms:.2e} {e_bias:.2e}")
        if e_max > worst[0]:
            worst = (e_max, worst[1], spec.name, worst[3])
        if e_rel > worst[1]:
            worst = (worst[0], e_rel, worst[2], spec.name)
        assert e_max < LAYER_BAR[dtype], (dtype, spec.name, e_max, e_rel)
    print(f"{dtype} hostile per-layer 320x240 (max_rel, elem, rms, bias):\n" + "\n".join(table))
    print(f"{dtype} hostile per-layer 320x240: worst max-abs/max-abs {worst[0]:.2e} ({worst[2]}), worst per-element {worst[1]:.2e} ({worst[3]})")
    assert worst[1] < LAYER_ELEM_BAR[dtype]
    if dtype in ("f32s", "f32x"):
        amax, wmax, sat = c.split_range()
        print(f"   split range monitor: max |activation| {amax:.3g}, max |Winograd input| {wmax:.3g}, saturated {sat}")
        assert not sat
    c.close()


def test_whole_frame_1080p_on_hostile_parameters(hostile_blob, ref1080, oracle):
    fr, ref, ref_aux = ref1080
    for dtype in ("f32", "f32s", "f32x", "f16", "f16hl"):
        c = Context(device=0, dtype=dtype)
        m = Model(c).control(ModelCmd.LoadBlob(hostile_blob))
        rgba, _ = FramePath(c).advance(fr, 1.0)
        lo, la = m.lowres()
        e_max, e_rel, e_rms, e_bias = A.grade(lo, ref, dtype, "hostile/logits1080", "1920x1080 out")
        a_max, a_rel, a_rms, a_bias = A.grade(la, ref_aux, dtype, "hostile/logits1080", "1920x1080 aux")
        print(f"{dtype} hostile 1920x1080: rms out {e_rms:.2e} aux {a_rms:.2e}, bias out {e_bias:.2e} aux {a_bias:.2e}")
        kr, _ = oracle.argmax(ref)
        kg, _ = oracle.argmax(lo)
        srt = np.sort(np.maximum(ref, 0.0), axis=0)
        gap = srt[-1] - srt[-2]
        bad = kr != kg
        unexplained = int((bad & (gap >= LOGIT_BAR[dtype] * np.abs(ref).max())).sum())
        print(f"{dtype} hostile 1920x1080: out {e_max:.2e} / {e_rel:.2e}, aux {a_max:.2e} / {a_rel:.2e} (max-abs/max-abs / per-element); "
              f"low-res class map differs on {int(bad.sum())} of {bad.size} pixels, {unexplained} outside the tolerance band")
        assert e_max < LOGIT_BAR[dtype] and a_max < LOGIT_BAR[dtype] and unexplained == 0
        assert e_rel < ELEM_BAR[dtype] and a_rel < ELEM_BAR[dtype]
        # the post stage stays bit-exact given the logits
        h, w = fr.shape[:2]
        assert (rgba == oracle.colorcode(oracle.upsample_bilinear(lo, h, w))).all()
        c.close()


def test_fast_modes_over_hostile_seeds(oracle):
    """f16hl (and f32x, f32s and f32 beside it) over six hostile parameter sets x two frames at 960x540 + one
    1920x1080 frame on a set other than the historical one, each against a float64 evaluation of the network, made once per case and
    shared by the modes: the four readings of tests/accuracy.py per case."""
    from oracle.infur_oracle import TorchModel

    worst = {dt: [0.0, 0.0] for dt in SEED_MODES}
    cases = [(sd, (540, 960), idx) for sd in H.SEEDS for idx in (2, 7)] + [(H.SEEDS[4], (1080, 1920), 2)]
    model64, last = None, None
    for (seed, base), (h, w), idx in cases:
        if last != (seed, base):
            blob = H.hostile_blob(seed=seed, base_seed=base)
            model64, last = TorchModel(blob, float64=True), (seed, base)
        fr = H.saturated_frame(h, w, index=idx)
        ref, ref_aux = (t.numpy() for t in model64.forward_lowres(oracle.pack_normalize(fr)))
        for dt in worst:
            c = Context(device=0, dtype=dt)
            m = Model(c).control(ModelCmd.LoadBlob(blob))
            rgba, _ = FramePath(c).advance(fr, 1.0)
            lo, la = m.lowres()
            where = f"seed {seed:#x} base {'lib' if base is None else hex(base)} {w}x{h} frame {idx}"
            (e, r, s, b), (ea, ra, sa, ba) = A.grade(lo, ref, dt, "hostile/seeds", where + " out"), A.grade(la, ref_aux, dt, "hostile/seeds", where + " aux")
            print(f"{dt} hostile {where}: {max(e, ea):.2e} ; {max(r, ra):.2e} ; rms {max(s, sa):.2e} ; bias {max(b, ba):.2e}")
            assert max(e, ea) < SEED_LOGIT_BAR[dt] and max(r, ra) < SEED_ELEM_BAR[dt], (dt, hex(seed), idx, e, ea, r, ra)
            worst[dt] = [max(worst[dt][0], e, ea), max(worst[dt][1], r, ra)]
            if dt == "f16hl":  # the post stage stays bit-exact given the logits
                assert (rgba == oracle.colorcode(oracle.upsample_bilinear(lo, h, w))).all()
            c.close()
    for dt, (a, b) in worst.items():
        print(f"{dt} over {len(cases)} hostile cases: worst max-abs/max-abs {a:.2e}, worst per-element {b:.2e}")
        assert a < LOGIT_BAR[dt]  # north_star's 1e-3, with room


def test_f32x_tiles_on_hostile_parameters(hostile_blob, ref1080, oracle):
    """INFUR_DTYPE_F32_SPLIT_FP8 with its two useful Winograd tiles at 1920x1080: F(4x4) holds VERDICT r3's 1e-2 per element
    (measured 7e-3), the F(6x6) default -- 7.5 % faster -- sits at the line (1.03e-2); both are 7-9x inside north_star's 1e-3."""
    fr, ref, ref_aux = ref1080
    for tile, elem_bar in ((4, 1e-2), (6, 1.5e-2)):
        c = Context(device=0, dtype="f32x", winograd_tile=tile)
        m = Model(c).control(ModelCmd.LoadBlob(hostile_blob))
        FramePath(c).advance(fr, 1.0)
        lo, la = m.lowres()
        cap = (None, elem_bar, None, None)  # (F(4x4)'s own, tighter per-element bar)
        e_max, e_rel, e_rms, e_bias = A.grade(lo, ref, "f32x", "hostile/logits1080", f"1920x1080 F({tile}x{tile}) out", cap=cap)
        a_max, a_rel, a_rms, a_bias = A.grade(la, ref_aux, "f32x", "hostile/logits1080", f"1920x1080 F({tile}x{tile}) aux", cap=cap)
        print(f"f32x F({tile}x{tile}) hostile 1920x1080: out {e_max:.2e} / {e_rel:.2e}, aux {a_max:.2e} / {a_rel:.2e}; rms {e_rms:.2e} / {a_rms:.2e}, bias {e_bias:.2e} / {a_bias:.2e}")
        assert max(e_max, a_max) < 3e-4 and max(e_rel, a_rel) < elem_bar
        c.close()
