"""Every conv layer of every float mode graded ALONE (tests/own_error.py): the device's output of a layer against the float64
evaluation of that one layer on the inputs the device itself stored, under the own/* bars of tests/accuracy.py -- 1.3 x the measured own
error: 2x to 180x below the */layer bars (which hold the error of up to 56 upstream layers) on the 1x1 kernels, the heads and F(2x2),
1.3x to 30x on the direct 3x3 kernels, and about equal to them on the F(4x4) / F(6x6) layers, whose own error IS the chain's.

Small shapes only, the two ragged sizes of accuracy.PLANT_SIZES (stride-8 maps 17 x 31 and 13 x 8: a tail tile and cut Winograd tiles at
every level): the friendly weights on the synthetic frame at 135 x 241, the historical hostile weights on the saturated frame at 97 x 61,
in every (mode, variant) an existing per-layer test forces through Context options, plus the f16 ResNet-101 with the 23 fused
conv3 + next conv1 launches forced.  Which own/wino* scope a variant reaches is read off the profile, never off the options.

Three planted faults (host arithmetic on the read-back tensors, no kernel altered): Q1 a dropped tap row on a border row, Q2 (f16) a
truncation where the kernel rounds, Q3 a tail tile that misses a K slice of a mid-network 1x1 -- graded the old way (against the oracle's
own chain, hostile/layer bars) and on the layer's own arithmetic; both sets of numbers are printed.  Recorded on an MI355X (max_rel,
elem, rms, bias): Q1 (0.56, 4.8, 0.18, 4.1e-3) and Q3 (7.5e-2, 3.4, 5.1e-2, 7.0e-4) in every mode -- the own bars reject them and so do
the chain bars, on all four readings: faults of that size needed no new bar.  Q2 graded the old way reads (1.13e-3, 5.5e-2, 7.2e-4,
8.3e-5) and PASSES the f16 chain bars (5.2e-3, 0.32, 1.9e-3, 1.7e-4); own/1x1 rejects it by bias (1.2e-4 against 4.4e-5), own16/1x1 by
elem, rms and bias.  (Q1 as first worded -- row 0 without kernel row 0 -- changes no bit on a pad-1 conv: own_error.Q1_KY.)"""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import hostile as H  # noqa: E402
import own_error as OE  # noqa: E402

from infur_amd import weights as W  # noqa: E402
from infur_amd.processors import Context, Model, ModelCmd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

OFF = 0xFFFFFFFF
# (mode, variant, Context options, the Winograd tile that must be reached -- None: no Winograd kernel may run)
VARIANTS = [
    ("f32", "direct", dict(winograd_min_cin=OFF), None),
    ("f32", "F2", dict(winograd_tile=2, winograd_min_cin=64), 2),
    ("f32", "F4", dict(winograd_tile=4, winograd_min_cin=64), 4),
    ("f32", "F6", dict(winograd_tile=6, winograd_min_cin=64), 6),
    ("f16hl", "direct", dict(winograd_min_cin=OFF), None),  # as test_hl_per_layer
    ("f16hl", "F4", dict(winograd_tile=4, winograd_min_cin=0), 4),
    ("f16hl", "F6", dict(winograd_tile=6, winograd_min_cin=0), 6),
    ("f32s", "default", dict(), 6),
    ("f32s", "direct", dict(winograd_min_cin=OFF), None),
    ("f32x", "F4", dict(winograd_tile=4), 4),
    ("f32x", "F6", dict(winograd_tile=6), 6),
    ("f16", "default", dict(), None),  # (the f16 mode has no Winograd form: wino_eligible)
]
SETS = ("friendly", "hostile")


@pytest.fixture(scope="module")
def sets(blob50, oracle):
    """weights -> (blob, frame, its normalised planes, TorchModel float64, the same with f16 weights), made once"""
    from oracle.infur_oracle import TorchModel

    out = {}
    for name, blob, fr in (("friendly", blob50, W.synth_frame(135, 241, index=135 + 241)), ("hostile", H.hostile_blob(), H.saturated_frame(97, 61))):
        m64 = TorchModel(blob, float64=True)
        out[name] = (blob, fr, oracle.pack_normalize(fr), m64, OE.f16_weight_model(m64))
    return out


def device_frame(blob, fr, mode, opts):
    c = Context(device=0, dtype=mode, keep_activations=True, profile=True, **opts)
    Model(c).control(ModelCmd.LoadBlob(blob)).advance(fr, [])
    return c


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("mode,variant,opts,tile", VARIANTS, ids=[f"{v[0]}-{v[1]}" for v in VARIANTS])
def test_every_layer_on_its_own_arithmetic(sets, mode, variant, opts, tile, which):
    blob, fr, chw, m64, m16 = sets[which]
    with device_frame(blob, fr, mode, opts) as c:
        rows = OE.grade_own(c, m64, chw, mode, variant, f"{which} {fr.shape[1]}x{fr.shape[0]}", model16=m16 if mode == "f16" else None)
    print(OE.format_table(rows, f"{mode} {variant} {which} {fr.shape[1]}x{fr.shape[0]}"))
    assert len(rows) == 57
    reached = {r["scope"] for r in rows if r["scope"].startswith("own/wino")}
    assert reached == ({f"own/wino{tile}"} if tile else set()), (mode, variant, reached)
    assert {"own/1x1", "own/direct", "own/head"} <= {r["scope"] for r in rows}
    OE.assert_table(rows)


R101_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import own_error as OE
from infur_amd import weights as W
from infur_amd.processors import Context, Model, ModelCmd
from oracle.infur_oracle import COracle, TorchModel
blob = W.synth_blob(depth=101)
fr = W.synth_frame(97, 61, index=97 + 61)
m64 = TorchModel(blob, float64=True)
with Context(device=0, dtype="f16", keep_activations=True, profile=True) as c:
    Model(c).control(ModelCmd.LoadBlob(blob)).advance(fr, [])
    pairs = sum(1 for r in c.profile() if r["kernel"] == "conv1x1_b2b_f16")
    rows = OE.grade_own(c, m64, COracle().pack_normalize(fr), "f16", "fused pairs", "R101 61x97", model16=OE.f16_weight_model(m64))
print(OE.format_table(rows, "f16 R101 fused pairs 61x97"))
print("RESULT " + json.dumps({"pairs": pairs, "rows": [[r["name"], r["scope"], r["kernel"], r["bad"], r["bad16"]] for r in rows]}))
"""


def test_resnet101_f16_with_the_fused_pairs_forced():
    """INFUR_B2B is read once per process: a child of its own, as in tests/test_gpu_b2b.py"""
    env = dict(os.environ)
    env["INFUR_B2B"] = "1"
    r = subprocess.run([sys.executable, "-c", R101_SCRIPT, ROOT], env=env, timeout=300, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    rows = res["rows"]
    assert res["pairs"] == 23 and len(rows) == 108
    fused = [x for x in rows if "conv1x1_b2b_f16" in x[2]]
    assert len(fused) == 46 and all(x[1] == "own/1x1" for x in fused)  # both halves of every pair
    assert not any(x[1].startswith("own/wino") for x in rows)
    bad = [(x[0], x[3], x[4]) for x in rows if x[3] or x[4]]
    assert not bad, bad


# ---- the planted faults ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain64(sets):
    """the float64 model's OWN chain on the hostile set: what the per-layer tests before this file grade against"""
    _, _, chw, m64, _ = sets["hostile"]
    taps = {}
    m64.forward_lowres(chw, taps=taps)
    return {k: v.numpy() for k, v in taps.items()}


@pytest.mark.parametrize("mode", A.MODES)
def test_planted_faults_miss_the_own_bars_and_what_the_chain_bars_say(sets, chain64, mode):
    blob, fr, chw, m64, m16 = sets["hostile"]
    with device_frame(blob, fr, mode, {}) as c:
        acts = OE.read_all(c, 50, fr.shape[:2])
        by_layer = OE.layer_records(c.profile(), m64.specs)
    taps64 = OE.forced_taps(m64, chw, acts)
    params = OE.params_of(blob)
    specs = {s.name: s for s in m64.specs}
    plants = [("Q1 (output row 0 without kernel row 1)", OE.Q1_LAYER, OE.plant_q1(acts, params, m64.specs)),
              ("Q3 (tail tile misses K 480..511)", OE.Q3_LAYER, OE.plant_q3(acts, params))]
    if mode == "f16":
        plants.append(("Q2 (truncated to f16, not rounded)", OE.Q2_LAYER, OE.plant_q2(taps64[OE.Q2_LAYER])))
        taps16 = OE.forced_taps(m16, chw, acts)
    slipped = []
    for what, layer, planted in plants:
        scope = OE.scope_of(specs[layer], by_layer[layer], acts[layer].shape[1:])[0]
        r_old0, r_old = A.readings(acts[layer], chain64[layer]), A.readings(planted, chain64[layer])
        r_own0, r_own = A.readings(acts[layer], taps64[layer]), A.readings(planted, taps64[layer])
        bad_old, bad_own = A.failures(r_old, mode, "hostile/layer"), A.failures(r_own, mode, scope)
        print(f"{mode} 61x97 {what} on {layer}:\n"
              f"   against the oracle's own chain: unplanted {A.fmt(r_old0)}, planted {A.fmt(r_old)}, hostile/layer bars {A.fmt(A.effective_bars(mode, 'hostile/layer'))}"
              f" -- {'REJECTED by ' + ', '.join(bad_old) if bad_old else 'PASSES'}\n"
              f"   on its own arithmetic:          unplanted {A.fmt(r_own0)}, planted {A.fmt(r_own)}, {scope} bars {A.fmt(A.effective_bars(mode, scope))}"
              f" -- {'REJECTED by ' + ', '.join(bad_own) if bad_own else 'PASSES'}")
        assert not A.failures(r_own0, mode, scope), A.message(r_own0, mode, scope, layer)
        if what.startswith("Q2"):
            s16 = scope.replace("own/", "own16/")
            r16 = A.readings(planted, taps16[layer])
            bad16 = A.failures(r16, mode, s16)
            print(f"   with the reference's weights in f16: planted {A.fmt(r16)}, {s16} bars {A.fmt(A.effective_bars(mode, s16))}"
                  f" -- {'REJECTED by ' + ', '.join(bad16) if bad16 else 'PASSES'}")
            assert bad16, f"{mode} {what}: passes the {s16} bars: {A.fmt(r16)}"
        assert bad_own, f"{mode} {what}: passes the {scope} bars: {A.fmt(r_own)}"
        if not bad_old:
            slipped.append(what[:2])
    print(f"{mode}: the chain bars let through {slipped or 'none'} of {[p[0][:2] for p in plants]}")
