"""Every tile form of the conv kernels, forced (INFUR_CONV_CFG) in every arithmetic mode, must PROVE that it ran and give the bits of
the mode's configuration 0 -- per layer on the unfused launches and on the fused product path with a reused arena, at sizes where
M = 1, M < BM, M is a whole number of tiles (the tail code must do nothing) and M is ragged against every tile -- and configuration 0
itself must agree with the float64 reference (the integer oracle for the quantised model) layer by layer at all of those sizes.
The three-byte mode runs every form with both K loops of conv_hl.hip (INFUR_HL_PIPE unset / = 0).  tests/forms.py holds the table
of forms, the sizes and the child process.

The tuner lets a forced form that is not a candidate for a layer fall back to the default SILENTLY (infur_tuner.cpp: pick_cfg), so
equal bits alone prove nothing: each case first finds its form's exact kernel name in the product path's profile and prints the
layers that carried it.  A form that runs on no layer at any size is a failure, not a skip.

Bars: tests/accuracy.py's scope "edge" -- four readings per layer and for the product path's logits, each at min(the bar before,
1.3 x measured) -- with the bars this file had before that table kept as caps of the max-abs reading (mode_bars, SIZE_BARS).  Those
were: the per-layer bar each mode's own suite states for this blob (max-abs error / max-abs reference per layer) -- REL_TOL of
test_gpu_parity.py (f32), SPLIT_TOL and FP8X_TOL of test_gpu_split.py (f32s, f32x), F16_TOL of test_gpu_f16_r101.py (f16),
HL_LAYER_TOL of test_gpu_hl.py (f16hl); i8 is bit-exact against oracle/infur_qoracle.py as in test_gpu_quant.py.  No layer is left out:
the float64 reference of every one of the 57 layers has max-abs >= 0.22 at all five sizes (backbone.layer1.0.conv2 at 1x1 the
smallest), so the denominator is never degenerate.

Measured on an MI355X, worst layer per mode at 135x241 / 97x61 / 128x128 / 3x5 / 1x1 (configuration 0, per-layer read-back):
  f32    8.5e-6 / 1.3e-5 / 1.1e-5 / 5.1e-6 / 4.8e-6    bar 1e-3
  f32s   5.8e-6 / 1.0e-5 / 6.5e-6 / 4.3e-6 / 4.2e-6    bar 3e-5
  f32x   3.7e-4 / 5.3e-4 / 5.8e-4 / 1.6e-4 / 1.6e-4    bar 5e-4 (1e-3 at 97x61 and 128x128, see below)
  f16    2.1e-3 / 1.8e-3 / 1.7e-3 / 1.3e-3 / 1.5e-3    bar 5e-3
  f16hl  3.8e-4 / 4.8e-4 / 5.6e-4 / 1.7e-4 / 1.9e-4    bar 1e-3
  i8     0 everywhere (bit-exact)
Nothing special happens at the one-pixel maps: 3x5 and 1x1 are the SMALLEST errors of every mode.

f32x: test_gpu_split.py states FP8X_TOL = 5e-4 for the LOGITS (measured 2-3e-4) and no per-layer bar; it is the bar used here.  Two
sizes exceed it, 97x61 with 5.31e-4 on backbone.layer4.1.conv2 and 128x128 with 5.83e-4 on backbone.layer3.1.conv2.  Both are dilated
3x3 convs evaluated as Winograd F(6x6), whose output transform amplifies the ~2^-13 error of the e5m2 cross terms (test_gpu_split.py:
F(6x6) against the direct convs).  It is the arithmetic, not a kernel: f16hl -- the same products in its own kernel -- has its worst
error on the same two layers with 4.79e-4 / 5.63e-4 (its stated per-layer bar is 1e-3), f32s -- f32x's own kernel with exact cross
terms -- measures 1e-5 there, all thirteen forms give configuration 0's bytes, and the logits stay at 2-3e-4.  Those two sizes get
min(2 x measured, north_star's 1e-3) = 1e-3; the other three keep 5e-4.
"""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import accuracy as A  # noqa: E402
import forms as F  # noqa: E402

gpu = pytest.mark.gpu

# north_star's bar for the f32-grade modes: no size-specific bar of SIZE_BARS may exceed it
NORTH_STAR = 1e-3
F32_GRADE = ("f32", "f32s", "f32x", "f16hl")
# (mode, (h, w)) -> bar, for a size whose MEASURED per-layer error exceeds the mode's stated bar for reasons of arithmetic: at most
# twice the measured value (recorded, with the reason, in the docstring above)
SIZE_BARS = {("f32x", (97, 61)): 1e-3, ("f32x", (128, 128)): 1e-3}


def mode_bars():
    """the per-layer bars as the modes' own suites stated them before tests/accuracy.py's table (whose scope "edge" grades all four
    readings at min(these, 1.3 x measured)): they stay as caps of the max-abs reading, per size (SIZE_BARS)"""
    import test_gpu_f16_r101
    import test_gpu_hl
    import test_gpu_parity
    import test_gpu_split

    return {"f32": test_gpu_parity.REL_TOL, "f32s": test_gpu_split.SPLIT_TOL, "f32x": test_gpu_split.FP8X_TOL,
            "f16": test_gpu_f16_r101.F16_TOL, "f16hl": test_gpu_hl.HL_LAYER_TOL}


rel_err = A.rel_err  # (one definition: tests/accuracy.py::readings)


# ---- what needs no GPU (tests/forms.py against the library's own table: tests/test_conv_forms_cpu.py) -------------------------------
def test_size_bars_stay_under_north_star():
    bars = mode_bars()
    assert set(bars) == set(F.MODES) - {"i8"}
    for (mode, size), bar in SIZE_BARS.items():
        assert size in F.SIZES and mode in bars
        assert mode not in F32_GRADE or bar <= NORTH_STAR, (mode, size, bar)


# ---- the shared runs and references -------------------------------------------------------------------------------------------------
class Shared:
    """the configuration-0 run of each mode (made once, kept for the module) and the references (made once, never changed)"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.base = {}
        self.digests = {}
        self.qblob_path = ""
        self.taps = None
        self.qtaps = None
        self.t0 = time.perf_counter()

    def path(self, mode, cfg, plain):
        return str(self.tmp / f"{mode}_cfg{cfg}{'_plain' if plain else ''}.npz")

    def qblob(self):
        if not self.qblob_path:
            from oracle import infur_qoracle as Q

            p = str(self.tmp / "qblob.bin")
            with open(p, "wb") as f:
                f.write(Q.synth_qblob())
            self.qblob_path = p
        return self.qblob_path

    def run(self, mode, cfg, plain):
        return F.run_child(mode, cfg, plain, self.path(mode, cfg, plain), self.qblob() if mode == "i8" else "")

    def baseline(self, mode):
        """the mode's configuration 0 (f16hl: with the pipelined K loop)"""
        if mode not in self.base:
            self.base[mode] = self.run(mode, 0, False)
        return self.base[mode]

    def float_taps(self, oracle):
        """size -> layer -> float64 reference, plus out_low / aux_low"""
        if self.taps is None:
            from infur_amd import weights as W
            from oracle.infur_oracle import TorchModel

            tm = TorchModel(W.synth_blob(), float64=True)
            self.taps = {}
            for h, w in F.SIZES:
                t = {}
                lo, la = tm.forward_lowres(oracle.pack_normalize(W.synth_frame(h, w, index=h + w)), taps=t)
                t = {k: v.numpy() for k, v in t.items()}
                t["out_low"], t["aux_low"] = lo.numpy(), la.numpy()
                self.taps[(h, w)] = t
        return self.taps

    def quant_taps(self, oracle):
        if self.qtaps is None:
            from infur_amd import weights as W
            from oracle import infur_qoracle as Q

            blob = open(self.qblob(), "rb").read()
            self.qtaps = {}
            for h, w in F.SIZES:
                t = {}
                lo, la = Q.qforward(blob, oracle.pack_normalize(W.synth_frame(h, w, index=h + w)), t)
                t["out_low"], t["aux_low"] = lo, la
                self.qtaps[(h, w)] = t
        return self.qtaps


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    s = Shared(tmp_path_factory.mktemp("forms"))
    yield s
    print(f"\ntest_gpu_forms.py: {time.perf_counter() - s.t0:.0f} s from the first case to the last")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def check_form_ran(run, mode, cfg, plain):
    """the forced form's exact kernel name is in the product path's profile; which layers carried it"""
    want = F.expected_kernel(mode, cfg, plain)
    carried = {}
    for size in F.SIZES:
        recs = run.kernels[F.tag(size)]
        carried[size] = [name for name, kernel in recs if kernel == want]
        if mode == "f16hl":
            dual = [name for name, _ in recs if name.endswith("conv3+downsample")]
            assert len(dual) == 4, (mode, cfg, size, dual)  # the two-source (DUAL) form ran
            tiled = [kernel for _, kernel in recs if kernel.startswith("conv_hl<") and "areg" not in kernel]
            assert tiled, (mode, cfg, size)
            if plain:  # the plain K loop really ran: every tiled launch says so
                assert all(k.endswith(",plain") for k in tiled), (mode, cfg, size, sorted(set(tiled)))
            else:
                assert not any("plain" in kernel for _, kernel in recs), (mode, cfg, size)
    layers = sorted({n for v in carried.values() for n in v})
    print(f"{mode} cfg {cfg} {want}: " + ", ".join(f"{F.tag(s)}: {len(v)} launches" for s, v in carried.items()))
    print(f"   layers: {' '.join(layers)}")
    assert layers, f"{mode}: forced configuration {cfg} ({want}) ran on no layer at any of {F.SIZES}: " \
                   f"kernels seen {sorted({k for v in run.kernels.values() for _, k in v})}"


def check_equal(ref, got, what):
    """per-layer read-back and product path, separately: byte for byte"""
    assert sorted(ref.keys()) == sorted(got.keys())
    bad_l = F.byte_differences(ref, got, "L/")
    bad_p = F.byte_differences(ref, got, "P/")
    assert not bad_l, f"{what}: per-layer read-back differs from configuration 0 in (key, elements) {bad_l[:12]} ({len(bad_l)} tensors)"
    assert not bad_p, f"{what}: product path differs from configuration 0 in (key, elements) {bad_p[:12]}"


def grade_float(run, mode, taps, oracle, what=""):
    """configuration 0 against the float64 reference: every layer, every size, four readings (tests/accuracy.py, scope "edge");
    what: names the variant in a failure message"""
    from infur_amd import weights as W

    bars = mode_bars()
    failures = []
    for size in F.SIZES:
        bar = SIZE_BARS.get((mode, size), bars[mode])
        ref = taps[size]
        worst, wname, n = 0.0, "", 0
        for name in [s.name for s in W.graph(50)] + ["out_low", "aux_low"]:
            got = run[f"L/{F.tag(size)}/{name}"]
            assert got.shape == ref[name].shape, (mode, size, name, got.shape, ref[name].shape)
            assert np.abs(ref[name]).max() > 0.1, (size, name)  # (measured: >= 0.22 everywhere)
            cap = (bar, None, None, None)
            r = A.grade(got, ref[name], mode, "edge", f"{what}{F.tag(size)} {name}", cap=cap, check=False)
            e = r[0]
            n += 1
            if e > worst:
                worst, wname = e, name
            if A.failures(r, mode, "edge", cap):
                failures.append(A.message(r, mode, "edge", f"{what}{F.tag(size)} {name}", cap))
        assert n == 59
        # the product path (fused launches: another summation order): its logits, and the mask given its logits
        p = []
        for name in ("out_low", "aux_low"):
            r = A.grade(run[f"P/{F.tag(size)}/{name}"], ref[name], mode, "edge", f"{what}{F.tag(size)} product path {name}", cap=cap, check=False)
            p.append(r[0])
            if A.failures(r, mode, "edge", cap):
                failures.append(A.message(r, mode, "edge", f"{what}{F.tag(size)} product path {name}", cap))
        p_out, p_aux = p
        print(f"{mode} {F.tag(size)}: worst layer {worst:.2e} ({wname}), bar {bar:g}; product path logits out {p_out:.2e} aux {p_aux:.2e}")
        h, w = size
        assert (run[f"P/{F.tag(size)}/rgba"] == oracle.colorcode(oracle.upsample_bilinear(run[f"P/{F.tag(size)}/out_low"], h, w))).all(), (mode, size)
    assert not failures, f"{mode}: over the bar:\n" + "\n".join(failures)


def grade_quant(run, qtaps, oracle):
    """the quantised model: every layer's bytes, the dequantised logits and the mask equal the integer oracle's"""
    from infur_amd import weights as W

    for size in F.SIZES:
        ref = qtaps[size]
        n = 0
        for spec in W.graph(50):
            if spec.role in ("cls", "auxcls"):
                continue  # the logit convs leave the stack dequantised: compared below
            got, want = run[f"L/{F.tag(size)}/{spec.name}"], ref[spec.name]
            assert got.shape[1:] == want.shape[1:] and got.shape[0] >= want.shape[0], (size, spec.name)
            assert (got[: want.shape[0]] == want.astype(np.float32)).all(), (size, spec.name, int((got[: want.shape[0]] != want).sum()))
            assert (got[want.shape[0]:] == 0).all(), (size, spec.name)  # channel padding of the 64-channel tensors
            n += 1
        assert n == 55
        h, w = size
        for path in ("L", "P"):
            lo, la = run[f"{path}/{F.tag(size)}/out_low"], run[f"{path}/{F.tag(size)}/aux_low"]
            assert (lo.view(np.uint32) == ref["out_low"].view(np.uint32)).all() and (la.view(np.uint32) == ref["aux_low"].view(np.uint32)).all(), (path, size)
        assert (run[f"P/{F.tag(size)}/rgba"] == oracle.colorcode(oracle.upsample_bilinear(ref["out_low"], h, w))).all(), size
        print(f"i8 {F.tag(size)}: 55 layers, logits and mask bit-exact against the integer oracle (worst error 0)")


@gpu
@pytest.mark.parametrize("mode,cfg,plain", F.cases(), ids=[f"{m}-cfg{k}{'-plain' if p else ''}" for m, k, p in F.cases()])
def test_forced_form_ran_and_gives_configuration_0s_bits(shared, oracle, mode, cfg, plain):
    if F.FATAL:
        pytest.fail(f"not started: an earlier child of this module ended badly ({F.FATAL[0]})")
    base = shared.baseline(mode)
    is_base = cfg == 0 and not plain
    run = base if is_base else shared.run(mode, cfg, plain)
    try:
        check_form_ran(run, mode, cfg, plain)
        if is_base:
            if mode == "i8":
                grade_quant(run, shared.quant_taps(oracle), oracle)
            else:
                grade_float(run, mode, shared.float_taps(oracle), oracle)
        else:
            check_equal(base, run, f"{mode} cfg {cfg}{' plain' if plain else ''}")
        if mode == "f16hl":  # the plain loop against the pipelined loop of the SAME form (cfg 0: `base` is that run)
            if not plain:
                shared.digests[cfg] = F.digests(run)
            elif cfg != 0:
                if cfg not in shared.digests:  # (the pipelined case of this form was not run before this one: a second child)
                    piped = shared.run(mode, cfg, False)
                    try:
                        shared.digests[cfg] = F.digests(piped)
                    finally:
                        piped.discard()
                mine = F.digests(run)
                bad = sorted(k for k in mine if mine[k] != shared.digests[cfg].get(k))
                assert not bad and len(mine) == len(shared.digests[cfg]), f"f16hl cfg {cfg}: plain K loop differs from the pipelined one in {bad[:12]}"
    finally:
        if not is_base:
            run.discard()
