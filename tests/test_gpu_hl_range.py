"""The range monitor of INFUR_DTYPE_F16_HL ("f16hl"; infur_hl_monitor_enable / infur_hl_range, ABI 7): opt-in, it records what the
splits of the six producers of three-byte tensors saw -- max |activation|, max |Winograd-domain input| (unscaled), whether the upper
clamp changed a value (beyond kHlHiMax = 65520, +inf included), whether a NaN arrived -- accumulated over every forward until read.
With the monitor off every kernel runs as before; with it on the stored bits do not change either."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, InfurError, Model, ModelCmd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from history import stem_gain_blob  # noqa: E402

pytestmark = pytest.mark.gpu

HL_HI_MAX = 65520.0  # hl_format.h: kHlHiMax


def bits(r):
    """an HlRange as comparable bit patterns"""
    return (int(np.float32(r.act_amax).view(np.uint32)), int(np.float32(r.wino_amax).view(np.uint32)), r.saturated, r.nan_seen)


def test_hl_monitor_mode_gating(blob50):
    for dtype in ("f32", "f32s", "f16"):
        with Context(device=0, dtype=dtype) as c:
            with pytest.raises(InfurError):
                c.set_hl_monitor(True)
    with Context(device=0, dtype="f16hl") as c:
        Model(c).control(ModelCmd.LoadBlob(blob50))
        with pytest.raises(InfurError):
            c.hl_range()
        c.set_hl_monitor(True)
        assert bits(c.hl_range()) == (0, 0, False, False)  # nothing run yet
        c.set_hl_monitor(False)
        with pytest.raises(InfurError):
            c.hl_range()


def test_hl_monitor_in_range_matches_read_back(blob50):
    """act_amax is the largest |value| of the three-byte activations.  The monitored and the kept sets differ in one form: with
    keep_activations the stem is kept as f32 (the exact stem) and its max-pool is what is converted to three bytes (and monitored);
    the stem is ReLU'd and every stem pixel lies in some pooling window, so the two maxima are the same value.  The two classifier
    outputs are f32 logits: never split, not monitored, skipped here."""
    fr = W.synth_frame(135, 241, index=5)
    for min_cin, wino in ((0, True), (0xFFFFFFFF, False)):
        c = Context(device=0, dtype="f16hl", keep_activations=True, winograd_min_cin=min_cin, hl_monitor=True)
        m = Model(c).control(ModelCmd.LoadBlob(blob50))
        m.advance(fr, [])
        r = c.hl_range()
        assert not r.saturated and not r.nan_seen
        if wino:
            assert r.wino_amax > 0
        else:
            assert r.wino_amax == 0
        if not wino:
            c.close()
            continue
        kept = 0.0
        for i, spec in enumerate(W.graph(50)):
            if spec.role in ("cls", "auxcls"):
                continue
            buf = np.empty(spec.cout * 135 * 241, np.float32)
            cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            c.check(c.L.infur_debug_read_activation(c.h, i, buf.ctypes.data, buf.size, C.byref(cc), C.byref(hh), C.byref(ww)))
            kept = max(kept, float(np.abs(buf[: cc.value * hh.value * ww.value]).max()))
        print(f"f16hl monitor: act_amax {r.act_amax:.6g}, kept max {kept:.6g}, wino_amax {r.wino_amax:.6g}")
        assert abs(r.act_amax - kept) <= 1e-3 * kept
        c.close()


def test_hl_monitor_reports_saturation():
    """the stem-gain ladder of tests/test_gpu_hl.py::test_hl_large_and_small_values: only x10^4 leaves the format's range"""
    fr = W.synth_frame(64, 96, index=2)
    for gain, sat in ((2.0 ** -8, False), (100.0, False), (1.0e4, True)):
        with Context(device=0, dtype="f16hl", hl_monitor=True) as c:
            m = Model(c).control(ModelCmd.LoadBlob(stem_gain_blob(gain)))
            FramePath(c).advance(fr, 1.0)
            lo, _ = m.lowres()
            r = c.hl_range()
            print(f"stem x{gain:g}: {r}")
            assert r.saturated == sat and not r.nan_seen
            assert np.isfinite(lo).all()
            if sat:
                assert r.act_amax > HL_HI_MAX


def test_hl_monitor_reports_nan_and_pins_todays_result():
    """NaN in one output channel's bias of a ReLU'd 1x1 conv is stored as 0 (the ReLU is the split's lower clamp), exactly like a
    bias of -1e30: same logits and mask byte for byte; only the monitor tells them apart"""
    fr = W.synth_frame(96, 128, index=1)
    res = {}
    for tag, val in (("nan", np.float32(np.nan)), ("neg", np.float32(-1e30))):
        tensors = []
        for s, w, b in W.synth_tensors(depth=50):
            if s.name == "backbone.layer2.0.conv1":
                assert s.relu and s.k == 1
                b = b.copy()
                b[7] = val
            tensors.append((s, w, b))
        with Context(device=0, dtype="f16hl", hl_monitor=True) as c:
            m = Model(c).control(ModelCmd.LoadBlob(W.pack_blob(tensors, 50, W.NUM_CLASSES, True)))
            rgba, _ = FramePath(c).advance(fr, 1.0)
            lo, la = m.lowres()
            res[tag] = (rgba, lo, la, c.hl_range())
    rn, rg = res["nan"][3], res["neg"][3]
    assert rn.nan_seen and not rn.saturated
    assert not rg.nan_seen
    for k in range(3):
        assert (res["nan"][k].view(np.uint8) == res["neg"][k].view(np.uint8)).all(), k


SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd
blob = W.synth_blob()
out = {}
c = Context(device=0, dtype="f16hl")
m = Model(c).control(ModelCmd.LoadBlob(blob))
for on in (0, 1):
    if on:
        c.set_hl_monitor(True)
    for i, (h, w) in enumerate(((135, 241), (97, 61))):
        fr = W.synth_frame(h, w, index=4 + i)
        rgba, _ = FramePath(c).advance(fr, 1.0)
        lo, la = m.lowres()
        out[f"lo{i}_{on}"] = lo; out[f"la{i}_{on}"] = la; out[f"rgba{i}_{on}"] = rgba
        if on:
            r = c.hl_range()
            out[f"r{i}"] = np.array([np.float32(r.act_amax).view(np.uint32), np.float32(r.wino_amax).view(np.uint32), r.saturated, r.nan_seen], np.uint32)
c.close()
np.savez(sys.argv[2], **out)
"""


def test_hl_monitor_changes_no_bits_and_ignores_the_tile_form(tmp_path):
    """forced tile forms (INFUR_CONV_CFG: 0 = 128x128, 11 = 256x256, 16 / 17 = the two-workgroup forms) and autotuned: the monitor
    on gives the bits of the monitor off, and the same monitor values in every form"""
    def run(cfg):
        path = str(tmp_path / f"cfg{cfg}.npz")
        env = dict(os.environ)
        env.pop("INFUR_CONV_CFG", None)
        if cfg is not None:
            env["INFUR_CONV_CFG"] = str(cfg)
        subprocess.run([sys.executable, "-c", SCRIPT, ROOT, path], check=True, env=env, timeout=300)
        return np.load(path)

    ref = None
    for cfg in (0, 11, 16, 17, None):
        got = run(cfg)
        for i in range(2):
            for k in ("lo", "la", "rgba"):
                assert (got[f"{k}{i}_0"].view(np.uint8) == got[f"{k}{i}_1"].view(np.uint8)).all(), (cfg, k, i)
            assert got[f"r{i}"][0] > 0 and got[f"r{i}"][2] == 0 and got[f"r{i}"][3] == 0
        if ref is None:
            ref = got
        for i in range(2):
            assert (got[f"r{i}"] == ref[f"r{i}"]).all(), (cfg, i, got[f"r{i}"], ref[f"r{i}"])


def test_hl_monitor_accumulates_until_read(blob50):
    fa, fb = W.synth_frame(64, 96, index=1), W.synth_frame(80, 112, index=6)
    with Context(device=0, dtype="f16hl", hl_monitor=True) as c:
        Model(c).control(ModelCmd.LoadBlob(blob50))
        fp = FramePath(c)
        fp.advance(fa, 1.0)
        r1 = c.hl_range()
        fp.advance(fb, 1.0)
        r2 = c.hl_range()
        assert bits(c.hl_range()) == (0, 0, False, False)  # a read straight after a read
        fp.advance(fa, 1.0)
        fp.advance(fb, 1.0)
        r12 = c.hl_range()
        fp.advance_batch([fa, fb], 1.0)
        rb = c.hl_range()
        assert bits(c.hl_range()) == (0, 0, False, False)
    want = (max(bits(r1)[0], bits(r2)[0]), max(bits(r1)[1], bits(r2)[1]), r1.saturated or r2.saturated, r1.nan_seen or r2.nan_seen)
    assert bits(r1) != bits(r2)  # two frames that differ
    assert bits(r12) == want and bits(rb) == want


def test_hl_monitor_under_graph_replay():
    blob = stem_gain_blob(1.0e4)
    fr = W.synth_frame(64, 96, index=2)
    with Context(device=0, dtype="f16hl", hl_monitor=True) as e:
        Model(e).control(ModelCmd.LoadBlob(blob))
        FramePath(e).advance(fr, 1.0)
        eager = e.hl_range()
    assert eager.saturated
    with Context(device=0, dtype="f16hl", hl_monitor=True, graph_replay=True) as c:
        Model(c).control(ModelCmd.LoadBlob(blob))
        fp = FramePath(c)
        for _ in range(20):
            fp.advance(fr, 1.0)
            if c.graph_stats()[1] > 0:
                break
        assert c.graph_stats()[1] > 0, c.graph_stats()
        c.hl_range()
        replays = c.graph_stats()[1]
        fp.advance(fr, 1.0)
        assert c.graph_stats()[1] == replays + 1
        r = c.hl_range()
        assert r.saturated and bits(r) == bits(eager)
        c.set_hl_monitor(False)
        assert c.graph_stats()[2] == 0
        fp.advance(fr, 1.0)
        c.set_hl_monitor(True)
        assert c.graph_stats()[2] == 0
