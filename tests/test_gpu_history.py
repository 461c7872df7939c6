"""A frame's bits must not depend on what its context ran before ("Arena": the history invariant).

Every case runs a TARGET frame in a context that has run nothing else and in a context that tests/history.py has walked through
larger frames, near-size frames, same-size frames of other content and a 10^4 times louder model -- the library's own earlier
frames, through the public API, are what leaves stale bytes in the never-cleared activation pool, in the lo planes of the
three-byte mode, in the staging buffers that only grow.  All tile configurations give the same bits in this project
(tests/test_gpu_conv_configs.py, test_gpu_hl.py, test_gpu_halo.py), so every comparison here is of bytes: logits, full-resolution
planes, mask, scaled frame, every kept activation.  The one tolerance is the oracle comparison of the fresh result, at the bar the
mode's own test file states -- "all equal" must not be able to mean "all equally wrong".
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import accuracy as A  # noqa: E402
import history as H  # noqa: E402
from test_gpu_f16_r101 import F16_TOL  # noqa: E402
from test_gpu_hl import HL_TOL  # noqa: E402
from test_gpu_parity import REL_TOL  # noqa: E402
from test_gpu_split import FP8X_TOL, SPLIT_TOL  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd import weights as W  # noqa: E402

pytestmark = pytest.mark.gpu

# the old bars; the comparison itself is graded by tests/accuracy.py (four readings, scope "edge")
ORACLE_TOL = {"f32": REL_TOL, "f32s": SPLIT_TOL, "f32x": FP8X_TOL, "f16hl": HL_TOL, "f16": F16_TOL}  # i8: bit-exact (Q.qforward)
T0 = H.FULL_TARGET  # (75, 109)


def tag(size):
    return f"{size[0]}x{size[1]}"


def target_frame(size):
    return W.synth_frame(size[0], size[1], index=H.target_index(size))


rel_err = A.rel_err  # (one definition: tests/accuracy.py::readings)


@pytest.fixture(scope="module")
def qblob():
    from oracle import infur_qoracle as Q

    return Q.synth_qblob()


@pytest.fixture(scope="module")
def loud_blob():
    return H.stem_gain_blob(H.LOUD_GAIN)


class Blobs(dict):
    """mode -> (the model, the loud model or None); a failure report prints a test's arguments, and these are 140 MB each"""

    def __repr__(self):
        return f"<model blobs of {', '.join(self)}>"


@pytest.fixture(scope="module")
def blobs(blob50, qblob, loud_blob):
    return Blobs({m: (qblob, None) if m == "i8" else (blob50, loud_blob) for m in H.MODES})


@pytest.fixture(scope="module")
def fresh(blobs):
    """(mode, target) -> what a context that has run nothing else computes, once per module.  The (75, 109) result carries the
    full-resolution planes too (a second forward, after the first one's results were taken)."""
    cache = {}

    def get(mode, target):
        if (mode, target) not in cache:
            with H.context(mode) as c:
                m = H.load(c, blobs[mode][0])
                cache[(mode, target)] = H.run(c, m, target_frame(target), full=target == T0)
        return cache[(mode, target)]

    return get


def assert_same(ref, got, what):
    """`got` holds the same bytes as `ref` under every key it has (a stage that did not read the full-resolution planes has fewer)"""
    assert set(got) <= set(ref) and {"lo", "la", "rgba"} <= set(got), (what, sorted(got))
    diff = H.first_difference({k: ref[k] for k in ref if k in got}, got)
    assert diff is None, f"{what}: fresh against walked -- {diff}"


@pytest.mark.parametrize("target", H.TARGETS, ids=tag)
@pytest.mark.parametrize("mode", H.MODES)
def test_outputs_do_not_depend_on_history(mode, target, blobs, fresh, oracle):
    blob, loud = blobs[mode]
    ref = fresh(mode, target)
    with H.context(mode) as c:
        m = H.load(c, blob)
        walked = H.walk(c, m, target, blob, loud)
    stages = ["after BIG"] + [f"after NEAR {tag(n)}" for n in H.near_sizes(target)] + ["after SAME", "after BIG through the loud model"]
    assert len(walked) == len(stages)
    bad = []  # every stage is looked at before anything is asserted: the message says which poisons show through
    for stage, got in zip(stages, walked):
        assert set(got) <= set(ref) and {"lo", "la", "rgba"} <= set(got), (stage, sorted(got))
        diff = H.first_difference({k: ref[k] for k in ref if k in got}, got)
        if diff is not None:
            bad.append(f"fresh against {stage} -- {diff}")
    for stage, got in zip(stages[1:], walked[1:]):  # two different histories against each other
        diff = H.first_difference({k: walked[0][k] for k in got if k in walked[0]}, {k: got[k] for k in got if k in walked[0]})
        if diff is not None:
            bad.append(f"{stages[0]} against {stage} -- {diff}")
    assert not bad, f"{mode} {tag(target)}: " + "; ".join(bad)
    assert np.isfinite(ref["lo"]).all() and np.isfinite(ref["la"]).all()
    if target != T0:
        return
    # the full-resolution planes belong to this target's results, and the second forward left the same logits
    assert {"out", "aux"} <= set(ref) and {"out", "aux"} <= set(walked[0]) and {"out", "aux"} <= set(walked[-1])
    assert H.first_difference({"lo": ref["lo"], "la": ref["la"]}, {"lo": ref["lo_full"], "la": ref["la_full"]}) is None
    h, w = target
    fr = target_frame(target)
    if mode == "i8":
        from oracle import infur_qoracle as Q

        ref_lo, ref_aux = Q.qforward(blob, oracle.pack_normalize(fr))
        assert H.first_difference({"lo": ref_lo, "la": ref_aux}, {"lo": ref["lo"], "la": ref["la"]}) is None
        assert (ref["out"].view(np.uint32) == oracle.upsample_bilinear(ref_lo, h, w).view(np.uint32)).all()
    else:
        from oracle.infur_oracle import TorchModel

        tl, ta = TorchModel(blob).forward_lowres(oracle.pack_normalize(fr))
        cap = (ORACLE_TOL[mode], None, None, None)
        r_out = A.grade(ref["lo"], tl.numpy(), mode, "edge", f"{tag(target)} fresh out", cap=cap)
        r_aux = A.grade(ref["la"], ta.numpy(), mode, "edge", f"{tag(target)} fresh aux", cap=cap)
        e_out, e_aux = r_out[0], r_aux[0]
        print(f"{mode} {tag(target)}: fresh logits rel err out={e_out:.2e} aux={e_aux:.2e} (old bar {ORACLE_TOL[mode]:g}); (max_rel, elem, rms, bias) out {A.fmt(r_out)} aux {A.fmt(r_aux)}")
        assert e_out < ORACLE_TOL[mode] and e_aux < ORACLE_TOL[mode]
        assert (ref["out"].view(np.uint32) == oracle.upsample_bilinear(ref["lo"], h, w).view(np.uint32)).all()
    assert (ref["rgba"] == oracle.colorcode(oracle.upsample_bilinear(ref["lo"], h, w))).all()


def run_kept(c, m, mode, frame):
    """one frame of a keep_activations context, as the mode's own per-layer test runs it"""
    from infur_amd.processors import FramePath

    if mode == "i8":
        FramePath(c).advance(frame, 1.0)
    else:
        m.advance(frame, [])


@pytest.mark.parametrize("mode", H.MODES)
def test_every_kept_layer_is_history_independent(mode, blobs):
    """keep_activations: nothing is reused inside a frame, every buffer is reused from the frame before -- each tensor of the
    target lies in a buffer the SAME frame filled in the same layout, or the BIG frame filled beyond its end"""
    blob, _ = blobs[mode]
    fr = target_frame(T0)
    with H.context(mode, keep_activations=True) as c:
        m = H.load(c, blob)
        run_kept(c, m, mode, fr)
        clean = H.kept_layers(c)
        clean["out_low"], clean["aux_low"] = m.lowres()
    with H.context(mode, keep_activations=True) as c:
        m = H.load(c, blob)
        run_kept(c, m, mode, W.synth_frame(T0[0], T0[1], index=H.IDX_SAME))
        same = H.kept_layers(c)
        run_kept(c, m, mode, W.synth_frame(H.BIG[0], H.BIG[1], index=H.IDX_BIG))
        run_kept(c, m, mode, fr)
        dirty = H.kept_layers(c)
        dirty["out_low"], dirty["aux_low"] = m.lowres()
    assert list(clean)[:-2] == [s.name for s in W.graph(50)]
    diff = H.first_difference(clean, dirty)  # (in graph order: the first layer that differs is the one named)
    assert diff is None, f"{mode}: first layer that depends on the frames before -- {diff}"
    # the poison was one: the SAME frame's layers are other values in the same shapes
    assert all(same[k].shape == clean[k].shape for k in same)
    assert sum(1 for k in same if (same[k] != clean[k]).any()) == len(same)
    if mode == "i8":
        padded = 0
        for spec in W.graph(50):
            if spec.role in ("cls", "auxcls"):
                continue
            t = dirty[spec.name]
            assert t.shape[0] >= spec.cout
            assert (t[spec.cout:] == 0).all(), f"{spec.name}: channel padding is not zero after other frames"
            padded += t.shape[0] > spec.cout
        assert padded > 0  # (the 64-channel tensors are padded: the check above looked at something)


@pytest.mark.parametrize("tile", [2, 4, 6, "direct"])
@pytest.mark.parametrize("mode", ["f32", "f16hl"])
def test_winograd_tiles_are_history_independent(mode, tile, blobs):
    """every forced tile with winograd_min_cin=64 (the dilated convs included, as test_winograd_variants_per_layer), and no
    Winograd at all: BIG, NEAR, then the target, against a fresh context of the same options"""
    blob, _ = blobs[mode]
    kw = {"winograd_min_cin": 0xFFFFFFFF} if tile == "direct" else {"winograd_tile": tile, "winograd_min_cin": 64}
    from infur_amd.processors import FramePath

    near = H.near_sizes(T0)[0]
    with H.context(mode, **kw) as c:
        ref = H.run(c, H.load(c, blob), target_frame(T0))
    with H.context(mode, **kw) as c:
        m = H.load(c, blob)
        FramePath(c).advance(W.synth_frame(H.BIG[0], H.BIG[1], index=H.IDX_BIG), 1.0)
        FramePath(c).advance(W.synth_frame(near[0], near[1], index=H.IDX_NEAR), 1.0)
        got = H.run(c, m, target_frame(T0))
    assert_same(ref, got, f"{mode} tile {tile} {tag(T0)} after BIG, NEAR")


@pytest.mark.parametrize("mode", ["f32", "f16hl"])
def test_history_across_a_pool_trim(mode, blobs, fresh):
    """BIG, then the target five times: the fifth is the frame at which the runtime frees the buffers only BIG used and renumbers
    the slots; then BIG again (new buffers) and the target"""
    from infur_amd.processors import FramePath

    blob, _ = blobs[mode]
    ref = fresh(mode, T0)
    big = W.synth_frame(H.BIG[0], H.BIG[1], index=H.IDX_BIG)
    with H.context(mode) as c:
        m = H.load(c, blob)
        FramePath(c).advance(big, 1.0)
        for k in range(H.POOL_TRIM_AFTER + 1):
            assert_same(ref, H.run(c, m, target_frame(T0)), f"{mode} {tag(T0)} repeat {k} after BIG")
        FramePath(c).advance(big, 1.0)
        assert_same(ref, H.run(c, m, target_frame(T0)), f"{mode} {tag(T0)} after the trim and BIG")


@pytest.mark.parametrize("scale_mode", [_lib.SCALE_NEAREST, _lib.SCALE_BILINEAR], ids=["nearest", "bilinear"])
def test_scaled_frames_are_history_independent(scale_mode, blob50):
    """the staging buffers of the frame and of the scaled frame only grow: a 272x496 frame at 0.5 (the BIG network input), then
    150x218 at 0.5 (the (75, 109) one) -- its scaled frame and mask are those of a fresh context"""
    from infur_amd.processors import FramePath

    fr = W.synth_frame(2 * T0[0], 2 * T0[1], index=H.target_index(T0))
    with H.context("f32") as c:
        ref = H.run(c, H.load(c, blob50), fr, 0.5, want_scaled=True, scale_mode=scale_mode)
    assert ref["scaled"].shape == (T0[0], T0[1], 3) and ref["rgba"].shape == (T0[0], T0[1], 4)
    with H.context("f32") as c:
        m = H.load(c, blob50)
        rgba, scaled = FramePath(c, scale_mode).advance(W.synth_frame(2 * H.BIG[0], 2 * H.BIG[1], index=H.IDX_BIG), 0.5, want_scaled=True)
        assert scaled.shape == (H.BIG[0], H.BIG[1], 3)
        got = H.run(c, m, fr, 0.5, want_scaled=True, scale_mode=scale_mode)
    assert_same(ref, got, f"scale mode {scale_mode}: 150x218 at 0.5 after 272x496 at 0.5")
    assert "scaled" in got


@pytest.mark.parametrize("mode", ["f16hl", "f32x"])
def test_graph_replay_walk(mode, blobs, fresh):
    """the two modes tests/test_gpu_graph.py leaves out, and a graph context against a fresh EAGER one (there both contexts share
    their history): BIG until it replays, the target until it replays (through the pool trim), BIG eager again, the target"""
    from infur_amd.processors import FramePath

    blob, _ = blobs[mode]
    ref = fresh(mode, T0)
    big = W.synth_frame(H.BIG[0], H.BIG[1], index=H.IDX_BIG)
    with H.context(mode, graph_replay=True) as c:
        m = H.load(c, blob)
        fp = FramePath(c)
        k = 0
        for what, n in (("big", 10), ("target", 10), ("big", 3), ("target", 10)):
            for _ in range(n):
                if what == "big":
                    fp.advance(big, 1.0)
                else:
                    assert_same(ref, H.run(c, m, target_frame(T0)), f"{mode} graph replay, frame {k}")
                k += 1
        cap, rep, cached = c.graph_stats()
    assert cap >= 2 and rep > 0, (cap, rep, cached)
