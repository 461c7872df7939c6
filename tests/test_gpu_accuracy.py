"""The bars of tests/accuracy.py catch what the bars before them let through: two planted faults, at the ragged sizes of
tests/forms.py, in every float mode.  Everything here is host arithmetic on tensors a normal keep_activations run reads back -- the
classifier's input (the head's 3x3 conv output) and the low-res logits; no kernel is altered or run a second time.

  baseline  the unmodified logits pass bar(mode, "edge")
  P1        the 512 -> 21 classifier recomputed (float64 sums) with inputs and weights rounded to f16, put in the logits' place: what
            an f32-grade mode would give if its classifier ran in half precision.  Must be rejected in f32 and f32s; the old bars
            (max-abs / max-abs at 1e-3 in f32) pass it, which is printed.  In the other modes the readings are printed only.
  P2        the last M mod 128 pixels (the tail tile of the 128-row GEMM tiles) lose input channels 480..511: must be rejected in
            every float mode.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402

from infur_amd import weights as W  # noqa: E402
from infur_amd.processors import Context, Model, ModelCmd  # noqa: E402

pytestmark = pytest.mark.gpu

HEAD = [s.name for s in W.graph(50)].index("classifier.0")


@pytest.fixture(scope="module")
def refs(blob50, oracle):
    """size -> float64 low-res logits, made once"""
    from oracle.infur_oracle import TorchModel

    tm = TorchModel(blob50, float64=True)
    return {(h, w): tm.forward_lowres(oracle.pack_normalize(W.synth_frame(h, w, index=h + w)))[0].numpy() for h, w in A.PLANT_SIZES}


@pytest.mark.parametrize("size", A.PLANT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", A.MODES)
def test_planted_faults_are_rejected(blob50, refs, mode, size):
    h, w = size
    ref = refs[size]
    wc, bc = A.classifier_of(blob50)
    with Context(device=0, dtype=mode, keep_activations=True) as c:
        m = Model(c).control(ModelCmd.LoadBlob(blob50))
        m.advance(W.synth_frame(h, w, index=h + w), [])
        x = np.empty((512,) + ref.shape[1:], np.float32)
        cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        c.check(c.L.infur_debug_read_activation(c.h, HEAD, x.ctypes.data, x.size, C.byref(cc), C.byref(hh), C.byref(ww)))
        assert (cc.value, hh.value, ww.value) == x.shape
        lo = m.lowres()[0].copy()
    where = f"{h}x{w} keep_activations out_low"
    r0 = A.grade(lo, ref, mode, "edge", where, check=False)
    print(f"{mode} {where}: (max_rel, elem, rms, bias) {A.fmt(r0)}, bars {A.fmt(A.effective_bars(mode, 'edge'))}")
    assert not A.failures(r0, mode, "edge"), A.message(r0, mode, "edge", where)

    r1 = A.readings(A.plant_p1(x, wc, bc), ref)
    bad1 = A.failures(r1, mode, "edge")
    print(f"{mode} {h}x{w} P1 (half-precision classifier): {A.fmt(r1)} -- {'REJECTED by ' + ', '.join(bad1) if bad1 else 'passes'}; "
          f"the old bars {'pass' if A.old_bars_pass(r1, mode, 'edge') else 'reject'} it")
    if mode in ("f32", "f32s"):
        assert bad1, f"{mode} {h}x{w}: a half-precision classifier passes every bar: {A.fmt(r1)}"

    r2 = A.readings(A.plant_p2(lo, x, wc), ref)
    bad2 = A.failures(r2, mode, "edge")
    print(f"{mode} {h}x{w} P2 (tail tile misses K 480..511): {A.fmt(r2)} -- {'REJECTED by ' + ', '.join(bad2) if bad2 else 'passes'}; "
          f"the old bars {'pass' if A.old_bars_pass(r2, mode, 'edge') else 'reject'} it")
    assert bad2, f"{mode} {h}x{w}: a tail tile that misses a K slice passes every bar: {A.fmt(r2)}"
