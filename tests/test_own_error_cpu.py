"""tests/own_error.py and TorchModel.forward_lowres(forced=...) without a device: the forced walk is the unforced one when it is fed
its own tensors, an f32 evaluation of the network stands in for the device (own error at f32 rounding level on every layer), the three
planted faults move the readings of the planted layer only, and the scope classifier reads canned profile records."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import own_error as OE  # noqa: E402

from infur_amd import weights as W  # noqa: E402

H, WD = 97, 61  # accuracy.PLANT_SIZES[1]: stride-8 map 13 x 8, M = 104


@pytest.fixture(scope="module")
def blob():
    return W.synth_blob()


@pytest.fixture(scope="module")
def chw(oracle):
    return oracle.pack_normalize(W.synth_frame(H, WD, index=H + WD))


@pytest.fixture(scope="module")
def model64(blob):
    from oracle.infur_oracle import TorchModel

    return TorchModel(blob, float64=True)


@pytest.fixture(scope="module")
def standin(blob, chw):
    """the f32 TorchModel's taps as "device" tensors, and the model"""
    from oracle.infur_oracle import TorchModel

    tm = TorchModel(blob)
    taps = {}
    tm.forward_lowres(chw, taps=taps)
    return tm, {k: v.numpy() for k, v in taps.items()}


@pytest.fixture(scope="module")
def base(model64, chw, standin):
    """{layer: readings} of the stand-in against the forced float64 walk, and that walk's taps"""
    _, acts = standin
    taps64 = OE.forced_taps(model64, chw, acts)
    return {n: A.readings(acts[n], taps64[n]) for n in acts}, taps64


# ---- identity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aux", [True, False])
def test_forced_walk_fed_its_own_taps_is_the_unforced_walk(oracle, aux):
    from oracle.infur_oracle import TorchModel

    tm = TorchModel(W.synth_blob(aux=aux), float64=True)
    x = oracle.pack_normalize(W.synth_frame(41, 53, index=7))
    plain, again, forced = {}, {}, {}
    lo0, la0 = tm.forward_lowres(x, taps=plain)
    lo1, la1 = tm.forward_lowres(x, taps=again, forced=None)
    names = [s.name for s in W.graph(50, aux=aux)]
    assert list(plain) != [] and set(plain) == set(names) and ("aux_classifier.4" in plain) == aux and (la0 is None) == (not aux)
    for n in names:
        assert plain[n].dtype == again[n].dtype and (plain[n].numpy().view(np.uint64) == again[n].numpy().view(np.uint64)).all(), n
    lo2, la2 = tm.forward_lowres(x, taps=forced, forced={n: plain[n].numpy() for n in names})
    for n in names:  # every layer on its own unforced inputs: the same bits, the blocks with a downsample branch included
        assert (plain[n].numpy().view(np.uint64) == forced[n].numpy().view(np.uint64)).all(), n
    assert {"backbone.layer1.0.downsample.0", "backbone.layer1.0.conv3", "backbone.layer2.0.downsample.0"} <= set(names)
    for a, b in ((lo0, lo1), (lo0, lo2)) + (((la0, la1), (la0, la2)) if aux else ()):
        assert (a.numpy().view(np.uint64) == b.numpy().view(np.uint64)).all()
    # the f32 model, as bench.py's cpu_baseline and every existing caller use it: forced=None is the call without the argument
    t32 = TorchModel(W.synth_blob(aux=aux))
    a, _ = t32.forward_lowres(x)
    b, _ = t32.forward_lowres(x, forced=None)
    assert a.dtype == b.dtype and (a.numpy().view(np.uint32) == b.numpy().view(np.uint32)).all()


def test_a_forced_tensor_replaces_what_every_consumer_sees(model64, chw, base):
    """the four places a conv output is consumed: zero the tensor and the consumers' taps must be what bias alone gives"""
    _, fed = base
    taps64 = OE.forced_taps(model64, chw, fed)  # (any complete set of tensors will do as the inputs)
    specs = {s.name: s for s in model64.specs}
    for name, consumers in (("backbone.conv1", ["backbone.layer1.0.conv1", "backbone.layer1.0.downsample.0"]),  # through the max-pool
                            ("backbone.layer1.0.downsample.0", ["backbone.layer1.0.conv3"]),                       # the branch, before the add
                            ("backbone.layer1.0.conv3", ["backbone.layer1.1.conv1", "backbone.layer1.1.conv3"]),   # next conv and next residual
                            ("backbone.layer3.5.conv3", ["backbone.layer4.0.conv1", "backbone.layer4.0.downsample.0", "aux_classifier.0"])):  # layer3 -> the aux head
        forced = {k: np.array(v) for k, v in fed.items()}
        forced[name] = np.zeros_like(forced[name])
        taps = {}
        model64.forward_lowres(chw, taps=taps, forced=forced)
        assert (taps[name].numpy() == taps64[name]).all()  # computed and tapped as before
        for c in consumers:
            assert not (taps[c].numpy() == taps64[c]).all(), (name, c)
        moved = [k for k in taps64 if not (taps[k].numpy() == taps64[k]).all()]
        assert sorted(moved) == sorted(consumers), (name, moved)
    assert specs["backbone.layer3.5.conv3"].role == "conv3"
    with pytest.raises(AssertionError):
        OE.forced_taps(model64, chw, {k: v for k, v in fed.items() if k != "classifier.0"})


# ---- an f32 evaluation as the device -------------------------------------------------------------------------------------------------------
def test_f32_standin_has_own_error_at_f32_rounding_level(base):
    readings, _ = base
    bars = A.bar("f32", "friendly/layer")
    worst = [max(r[i] for r in readings.values()) for i in range(4)]
    for n, r in readings.items():
        print(f"   {n:34s} " + " ".join(f"{x:.2e}" for x in r))
    print(f"f32 stand-in, own error, worst over {len(readings)} layers {A.fmt(worst)}; friendly/layer f32 bars {A.fmt(bars)}")
    assert len(readings) == 57
    for x, b in zip(worst, bars):
        assert x < b / 10.0, (worst, bars)


# ---- the planted faults --------------------------------------------------------------------------------------------------------------
def faulty_standin(standin, chw, layer, planted):
    """the tensors a device with a fault in `layer` would have stored: the f32 walk, continued from the planted tensor"""
    tm, _ = standin
    taps = {}
    tm.forward_lowres(chw, taps=taps, forced={layer: planted})
    acts = {k: v.numpy() for k, v in taps.items()}
    acts[layer] = np.asarray(planted, np.float32)
    return acts


def test_q1_as_worded_changes_nothing_and_the_plant_drops_the_first_row_that_meets_data(blob, standin, model64):
    _, acts = standin
    params = OE.params_of(blob)
    spec, = [s for s in model64.specs if s.name == OE.Q1_LAYER]
    assert (spec.k, spec.pad, spec.dil, spec.stride) == (3, 1, 1, 1)  # output row 0, kernel row 0: input row -1, the padding
    w, b = params[OE.Q1_LAYER]
    exact = np.array(acts[OE.Q1_LAYER], np.float64)
    exact[:, 0, :] = np.maximum(OE.conv64(acts[OE.Q1_INPUT], w, b, spec), 0.0)[:, 0, :]
    assert (OE.plant_q1(acts, params, model64.specs, ky=0) == exact).all()
    d = OE.plant_q1(acts, params, model64.specs) - exact
    assert OE.Q1_KY == 1 and (d[:, 1:, :] == 0).all() and (d[:, 0, :] != 0).any()


@pytest.mark.parametrize("plant", ["Q1", "Q2", "Q3"])
def test_a_plant_moves_the_planted_layer_and_no_other(blob, standin, model64, chw, base, plant):
    readings, taps64 = base
    _, acts = standin
    params = OE.params_of(blob)
    if plant == "Q1":
        layer, planted = OE.Q1_LAYER, OE.plant_q1(acts, params, model64.specs)
    elif plant == "Q2":
        layer, planted = OE.Q2_LAYER, OE.plant_q2(taps64[OE.Q2_LAYER])
    else:
        layer, planted = OE.Q3_LAYER, OE.plant_q3(acts, params)
        assert planted.shape == (2048, 13, 8) and (13 * 8) % A.TAIL_TILE == 104
    faulty = faulty_standin(standin, chw, layer, planted)
    forced = OE.forced_taps(model64, chw, faulty)
    got = {n: A.readings(faulty[n], forced[n]) for n in faulty}
    level = [10.0 * max(r[i] for r in readings.values()) for i in range(4)]  # ten times the stand-in's worst layer: still f32 rounding level
    print(f"{plant} on {layer}: own error {A.fmt(got[layer])}, unplanted {A.fmt(readings[layer])}; the other layers stay under {A.fmt(level)}")
    for n, r in got.items():
        if n == layer:
            assert r[2] > 100.0 * readings[n][2] and r[0] > 10.0 * readings[n][0], (plant, r, readings[n])
        else:
            assert all(x < lv for x, lv in zip(r, level)), (plant, n, r, level)
    # graded the old way -- against the float64 model's OWN chain -- the fault is smeared over everything downstream
    names = [s.name for s in model64.specs]
    own = {}
    model64.forward_lowres(chw, taps=own)
    after = [s.name for s in model64.specs[names.index(layer) + 1:] if s.role != "down"][0]  # (the next conv that consumes it)
    old = A.readings(faulty[after], own[after].numpy())
    print(f"   the old way, one layer downstream ({after}): {A.fmt(old)} against an own error of {A.fmt(got[after])}")
    assert old[2] > 10.0 * got[after][2]


def test_q2_truncates_toward_zero():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10, -(1.0 + 3 * 2.0 ** -11), 65504.0, 0.0, 1e-9, -3.0])
    t = OE.plant_q2(x)
    assert (t == np.array([1.0, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 65504.0, 0.0, 0.0, -3.0])).all()
    r = np.random.default_rng(3).uniform(0.0, 8.0, 4096)
    t = OE.plant_q2(r)
    assert (t <= r).all() and (t.astype(np.float16) == t).all() and ((r - t) < 2.0 ** -8).all()


# ---- the classifier -------------------------------------------------------------------------------------------------------------------
def rec(name, kernel, flops=0.0, nbytes=0.0):
    return {"name": name, "kernel": kernel, "flops": flops, "bytes": nbytes, "variant": ""}


def test_the_scope_comes_from_the_kernels_that_ran():
    specs = W.graph(50)
    by = {s.name: s for s in specs}
    c2, head = by["backbone.layer2.1.conv2"], by["classifier.0"]
    hw = (13, 8)

    def wino(spec, mt, hl=""):
        planes, es = (mt + 2) ** 2, 3 if hl else 4
        pt = planes * OE.wino_tiles(hw[0], hw[1], spec.dil, mt)
        flops = 2.0 * pt * spec.cout * spec.cin  # (infur_capi.cpp: run_conv)
        nbytes = float(pt * spec.cin * es + pt * spec.cout * 4 + planes * spec.cout * spec.cin * es)
        return [rec(spec.name + "/in", "wino_input" + hl), rec(spec.name, "conv_hl<128,128>" if hl else "conv_igemm_f32<128,128>", flops, nbytes),
                rec(spec.name + "/out", "wino_output" + hl)]

    records = [rec("pre-proc", "pack_normalize"), rec("backbone.conv1", "stem_conv7x7"), rec("backbone.maxpool", "maxpool3x3s2"),
               rec("backbone.layer1.0.conv1", "conv_igemm_f32<64,64>"), rec("backbone.layer1.0.conv2", "conv3x3_f16<16x16,128,halo>"),
               rec("backbone.layer1.0.conv3", "conv1x1_f16<256,areg>"), rec("backbone.layer1.0.downsample.0", "conv_hl<128,areg>"),
               rec("backbone.layer2.0.conv2", "conv_igemm_f32s<256,128,1frag>"),
               rec("backbone.layer2.1.conv3+next.conv1", "conv1x1_b2b_f16"), rec("backbone.layer2.2.conv2", "conv_hl<256,128,4w>,plain"),
               rec("classifier.4", "conv_igemm_f32x<64,128>"), rec("aux_classifier.4", "conv_igemm_f16<128,64,1buf>"),
               rec("out.resize+colorcode", "post")]
    records += wino(c2, 4) + wino(head, 6, "_hl") + wino(by["backbone.layer4.0.conv2"], 2)
    got = OE.layer_records(records, specs)
    want = {"backbone.conv1": "own/direct", "backbone.layer1.0.conv1": "own/1x1", "backbone.layer1.0.conv2": "own/direct",
            "backbone.layer1.0.conv3": "own/1x1", "backbone.layer1.0.downsample.0": "own/1x1", "backbone.layer2.0.conv2": "own/direct",
            "backbone.layer2.1.conv3": "own/1x1", "backbone.layer2.2.conv1": "own/1x1", "backbone.layer2.2.conv2": "own/direct",
            "classifier.4": "own/head", "aux_classifier.4": "own/head", c2.name: "own/wino4", "classifier.0": "own/wino6",
            "backbone.layer4.0.conv2": "own/wino2"}
    for name, scope in want.items():
        assert OE.scope_of(by[name], got[name], hw)[0] == scope, name
        assert scope in A.SCOPES and scope in OE.OWN_SCOPES
    l4 = by["backbone.layer4.0.conv2"]  # dilation 2 at 13 x 8: F(2x2) and F(6x6) execute the same number of plane tiles
    assert l4.dil == 2 and 16 * OE.wino_tiles(13, 8, 2, 2) == 64 * OE.wino_tiles(13, 8, 2, 6) == 512
    assert "conv1x1_b2b_f16" in OE.scope_of(by["backbone.layer2.2.conv1"], got["backbone.layer2.2.conv1"], hw)[1]
    # every kernel name of tests/forms.py is known
    import forms

    for mode, table in forms.FORMS.items():
        for cfg in table:
            assert OE.kernel_kind(forms.expected_kernel(mode, cfg)) == "gemm"
            assert OE.kernel_kind(forms.expected_kernel(mode, cfg, plain=True)) == "gemm"
    # what it does not know fails loudly
    for bad in ("conv_igemm<?>", "conv_hl<?>", "some_new_kernel", "wino_input_f16", ""):
        with pytest.raises(ValueError):
            OE.kernel_kind(bad)
    with pytest.raises(ValueError):  # a layer without a record
        OE.scope_of(by["backbone.layer3.0.conv1"], got["backbone.layer3.0.conv1"], hw)
    with pytest.raises(ValueError):  # Winograd transforms around a GEMM of no tile's size
        OE.scope_of(c2, [rec(c2.name + "/in", "wino_input"), rec(c2.name, "conv_igemm_f32<64,64>", 12345.0, 678.0), rec(c2.name + "/out", "wino_output")], hw)
    with pytest.raises(ValueError):
        OE.layer_records([rec("backbone.layer1.0.conv3+something", "conv_igemm_f32<64,64>")], specs)


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_every_own_scope_is_asked_measured_and_had_no_bar():
    own = [s for s in A.SCOPES if s.startswith("own")]
    assert tuple(own) == OE.OWN_SCOPES + OE.OWN16_SCOPES
    for s in own:
        assert A.ASKED[s], s
        for m in A.ASKED[s]:
            assert A.WAS[(m, s)] == (None,) * 4
            assert (m, s) in A.MEASURED, (m, s)
            assert A.bar(m, s) == tuple(A.round_up(A.HEADROOM * x) for x in A.MEASURED[(m, s)])
    assert all(A.ASKED[s] == ("f16",) for s in OE.OWN16_SCOPES)
    for scope, bars in OE.HL_REST_CAP.items():  # a cap only ever tightens
        assert scope in OE.OWN_SCOPES and all(c is None or c <= b for c, b in zip(bars, A.bar("f16hl", scope)))
