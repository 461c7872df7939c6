"""Every kernel a launcher picks INSIDE one conv configuration -- from the size of the map or from an environment hook -- must prove
that it ran, at edge sizes, and give the bits of the mode's configuration 0.  tests/test_gpu_forms.py closed the gap between
configurations; its profile names say which configuration ran, not which of the configuration's two to four kernels.  Here each case
of forms.SUBFORM_CASES is one child process (every hook is read once into a static) of the forms child, under its per-child time
limit, its FATAL latch (after a child that ends by signal, abort or timeout, or reports a memory fault, nothing more is started) and
its no-retry rule, one after another.  Each case asserts, in this order:

1. the expected variant words (conv_forms.h: kVariantWords, through Context.profile()'s "variant") appear in the product path's
   profile -- printed with the layers that carried them; a word on no layer at any size fails the case -- and the words the hook
   excludes appear on none;
2. every L/ and P/ array equals the baseline's bytes (forms.byte_differences; for the 777x897 frame, whose 57 layers are 1.5 GB per
   run, the SHA-1 of every array): the baseline is INFUR_CONV_CFG=0 without any other hook, with the same Winograd tile at the same
   sizes;
3. the baselines at forms.SIZES are the runs tests/test_gpu_forms.py grades against the float64 reference; the baselines at the
   two sizes of this file (777x897, 64x256) are graded here the same way, every layer at the mode's own stated bar (F16_TOL).

The forced cases run at forms.SIZES: M = 1, M < BM, whole tiles (128x128: the layer1 map is exactly 4 x 256 pixels) and ragged tails
(135x241: 34 x 61 = 8 x 256 + 26).  The one natural case, 777x897, sets no hook besides INFUR_CONV_CFG, so the size rules
themselves choose: layer1's conv3 take the 256-pixel form of configuration 15 and all others the 128-pixel one, Cout 512 takes N
tiles of 128 in configuration 19 and Cout 256 tiles of 64 (figures: forms.NATURAL_SIZES, held on the CPU by
tests/test_conv_forms_cpu.py).  The other side of the quantised N-split rule (split 2 and 0) needs a map of 1080p class: it stays
with the CPU test of q8_nsplit_rule and the 1080p test of tests/test_gpu_quant.py.  64x256 is the smallest frame on which halo_plan
picks its 8 x 32 tiling.

Hooks that select code no default dispatch reaches -- INFUR_WINO_VEC=1 (f32x1), INFUR_WINO_VEC=2 (the non-vec4 F(2x2) / F(4x4)),
INFUR_STEM_F32=1 (stem_pool_kernel<_Float16>, the f32-MFMA stem under the split conv stack) -- are KEPT and covered here.

Not bit-identical by design: INFUR_STEM_F32=1.  The f32-MFMA stem computes the 7x7 conv in f32 where the mode's own fused stem
uses f16 operands (f16) or f16 hi + lo pairs (f32s), so the product path's pooled tensor differs in its last bits and every layer
after it.  The per-layer read-back (keep_activations) runs the UNFUSED stem in every case and must still equal the baseline byte for
byte; the product path's logits are graded against the float64 reference at the mode's stated bar (F16_TOL, SPLIT_TOL).
Measured, worse of out / aux at 135x241 / 97x61 / 128x128 / 3x5 / 1x1: f16 1.3e-3 / 1.1e-3 / 1.3e-3 / 1.3e-4 / 3.3e-5 (bar 5e-3),
f32s 3.9e-6 / 4.4e-6 / 5.0e-6 / 4.7e-7 / 1.4e-7 (bar 3e-5).

Not bit-identical by design either: INFUR_WINO_VEC=1, the 4-byte form of the F(6x6) transforms.  The transforms' translation unit is
built with floating-point contraction allowed (only the byte-exact stages are built without), and the compiler contracts the scalar
expressions of the f32x1 instantiation into other fused multiply-adds than the vector expressions of f32x2 / f32x4w (F(6x6) output
transform: 142 against 140 per channel) -- every result is the correctly rounded value of the same expression tree up to which
products are fused, f32-grade, not the same bits (129 of the 295 per-layer tensors differ from the baseline's, from the first
Winograd layer on).  It is graded layer by layer against the float64 reference at REL_TOL = 1e-3; measured worst layer at the five
sizes 9.3e-6 / 1.6e-5 / 1.1e-5 / 5.1e-6 / 4.8e-6, the baseline's own figures (test_gpu_forms.py: 8.5e-6 / 1.3e-5 / 1.1e-5 / ...).  The LDS
two-pass forms, the per-thread f32x2 form and the non-vec4 F(2x2) / F(4x4) forms ARE bit-identical to the default, on the same data.

The ablation hooks INFUR_STEM_ABL and INFUR_H4_ABL compute wrong results by design and are not run.

Measured on an MI355X: the baselines of this file's own sizes against the float64 reference, worst layer 1.83e-3 at 777x897
(backbone.layer3.1.conv2) and 1.78e-3 at 64x256 (backbone.layer4.0.conv1), bar 5e-3.  Wall time of the module: 30 children of
2.2-2.9 s (777x897: 3.8-4.3 s) and the float64 references, 99 s from the first case to the last.
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
import test_gpu_forms as TF  # noqa: E402
from test_gpu_forms import mode_bars, rel_err  # noqa: E402

gpu = pytest.mark.gpu

# The 777x897 child: 57 layers of 1.5 GB read back and hashed (the baseline writes them instead).  Measured on an MI355X: 4.3 s
# the baseline, 4.0 s and 3.8 s the two forced forms; the limit is five times the slowest, the margin forms.CHILD_TIMEOUT uses.
NATURAL_CHILD_SECONDS = 4.3
NATURAL_TIMEOUT = round(5 * NATURAL_CHILD_SECONDS)
TIMEOUTS = {"edge": None, "geom": None, "natural": NATURAL_TIMEOUT}  # None: forms.CHILD_TIMEOUT


class Shared:
    """the baseline run of each (mode, tile, sizes), made once and kept for the module"""

    def __init__(self, tmp):
        self.tmp = tmp
        self.base = {}
        self.qblob_path = ""
        self.forms = TF.Shared(tmp)  # (its float64 references of forms.SIZES, made once)
        self.t0 = time.perf_counter()

    def qblob(self):
        if not self.qblob_path:
            from oracle import infur_qoracle as Q

            self.qblob_path = str(self.tmp / "qblob.bin")
            with open(self.qblob_path, "wb") as f:
                f.write(Q.synth_qblob())
        return self.qblob_path

    def run(self, case):
        t = time.perf_counter()
        # the natural size: digests only, but the baseline keeps its arrays too (a second child of the same case would double its cost:
        # the parent hashes them itself)
        digest = case.sizes == "natural" and not case.baseline
        r = F.run_child(case.mode, case.cfg, False, str(self.tmp / (case.id + ".npz")), self.qblob() if case.mode == "i8" else "",
                        extra_env=case.env, tile=case.tile, sizes=None if case.sizes == "edge" else F.SIZE_SETS[case.sizes], digest=digest,
                        timeout=TIMEOUTS[case.sizes])
        print(f"{case.id}: child took {time.perf_counter() - t:.1f} s")
        return r

    def baseline(self, case):
        if case.key not in self.base:
            b = F.subform_baseline(case)
            self.base[case.key] = self.run(b)
        return self.base[case.key]


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    s = Shared(tmp_path_factory.mktemp("subforms"))
    yield s
    print(f"\ntest_gpu_subforms.py: {time.perf_counter() - s.t0:.0f} s from the first case to the last")


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def check_variants(run, case):
    """1.: the words the case must see, with the layers that carried them; the words it must never see"""
    sizes = F.SIZE_SETS[case.sizes]
    seen = {}  # word -> size -> layers
    for size in sizes:
        for layer, kernel, variant in run.variants[F.tag(size)]:
            for word in filter(None, variant.split(",")):
                seen.setdefault(word, {}).setdefault(size, []).append(layer)
    for word in sorted(seen):
        print(f"{case.id}: {word}: " + ", ".join(f"{F.tag(s)}: {len(v)}" for s, v in seen[word].items()))
        print(f"   layers: {' '.join(sorted({n for v in seen[word].values() for n in v}))}")
    for want in case.see:
        word, prefix = (want, "") if isinstance(want, str) else want
        layers = sorted({n for v in seen.get(word, {}).values() for n in v if n.startswith(prefix)})
        assert layers, f"{case.id}: variant {word!r} ran on no layer{' of ' + prefix if prefix else ''} at any of {sizes}: seen {sorted(seen)}"
    for word in case.never:
        assert word not in seen, f"{case.id}: variant {word!r} ran on {seen[word]} although the case excludes it"


def digest_of(a):
    import hashlib

    return np.frombuffer(hashlib.sha1(repr(a.shape).encode() + np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def check_equal(base, run, case, prefixes=("L/", "P/")):
    """2.: byte for byte (digest for digest where the child kept digests)"""
    if any(k.startswith("D/") for k in run.keys()):
        keys = sorted(k[2:] for k in run.keys())
        assert keys == sorted(base.keys()), case.id
        bad = [k for k in keys if k.startswith(prefixes) and not (digest_of(base[k]) == run["D/" + k]).all()]
        assert not bad, f"{case.id}: differs from configuration 0 in {bad[:12]} ({len(bad)} tensors)"
        return
    assert sorted(base.keys()) == sorted(run.keys()), case.id
    for prefix in prefixes:
        bad = F.byte_differences(base, run, prefix)
        assert not bad, f"{case.id}: {prefix} differs from configuration 0 in (key, elements) {bad[:12]} ({len(bad)} tensors)"


class _Grader(dict):
    """what TorchModel.forward_lowres is given as `taps`: grades each layer as its float64 reference arrives and keeps the error only
    (the references of a 777x897 frame are 2.9 GB)"""

    def __init__(self, run, size, mode, what, cap):
        super().__init__()
        self.mode, self.what, self.cap = mode, what, cap
        self.run, self.size, self.err, self.readings = run, size, {}, {}

    def __setitem__(self, name, ref):
        ref = ref.numpy() if hasattr(ref, "numpy") else ref
        got = self.run[f"L/{F.tag(self.size)}/{name}"]
        assert got.shape == ref.shape, (self.size, name, got.shape, ref.shape)
        assert np.abs(ref).max() > 0.1, (self.size, name)  # (the denominator is never degenerate: test_gpu_forms.py)
        self.readings[name] = A.grade(got, ref, self.mode, "edge", f"{self.what} {F.tag(self.size)} {name}", cap=self.cap, check=False)
        self.err[name] = self.readings[name][0]


def reference_logits(oracle, size):
    """float64 out_low / aux_low of one frame (small sizes: made per call)"""
    from infur_amd import weights as W
    from oracle.infur_oracle import TorchModel

    h, w = size
    lo, la = TorchModel(W.synth_blob(), float64=True).forward_lowres(oracle.pack_normalize(W.synth_frame(h, w, index=h + w)))
    return lo.numpy(), la.numpy()


def grade_baseline(run, case, oracle):
    """3.: a baseline at a size of this file against the float64 reference: every layer, the mode's stated bar"""
    from infur_amd import weights as W
    from oracle.infur_oracle import TorchModel

    bar = mode_bars()[case.mode]
    tm = TorchModel(W.synth_blob(), float64=True)
    for size in F.SIZE_SETS[case.sizes]:
        h, w = size
        cap = (bar, None, None, None)
        g = _Grader(run, size, case.mode, case.id, cap)
        lo, la = tm.forward_lowres(oracle.pack_normalize(W.synth_frame(h, w, index=h + w)), taps=g)
        g["out_low"], g["aux_low"] = lo, la
        assert len(g.err) == 59, len(g.err)
        worst = max(g.err, key=g.err.get)
        print(f"{case.id} {F.tag(size)}: worst layer {g.err[worst]:.2e} ({worst}), bar {bar:g}")
        over = [A.message(r, case.mode, "edge", f"{case.id} {F.tag(size)} {n}", cap) for n, r in g.readings.items() if A.failures(r, case.mode, "edge", cap)]
        assert not over, "over the bar:\n" + "\n".join(over)
        assert (run[f"P/{F.tag(size)}/rgba"] == oracle.colorcode(oracle.upsample_bilinear(run[f"P/{F.tag(size)}/out_low"], h, w))).all(), (case.id, size)


def grade_product_logits(run, case, oracle, refs):
    """a sub-form that is not bit-identical by design: the product path's logits against the float64 reference at the mode's bar"""
    bar = mode_bars()[case.mode]
    for size in F.SIZE_SETS[case.sizes]:
        h, w = size
        if size not in refs:
            refs[size] = reference_logits(oracle, size)
        cap = (bar, None, None, None)
        e_out = A.grade(run[f"P/{F.tag(size)}/out_low"], refs[size][0], case.mode, "edge", f"{case.id} {F.tag(size)} product path out_low", cap=cap)[0]
        e_aux = A.grade(run[f"P/{F.tag(size)}/aux_low"], refs[size][1], case.mode, "edge", f"{case.id} {F.tag(size)} product path aux_low", cap=cap)[0]
        print(f"{case.id} {F.tag(size)}: product path logits out {e_out:.2e} aux {e_aux:.2e}, bar {bar:g}")
        assert e_out < bar and e_aux < bar, (case.id, size, e_out, e_aux, bar)
        assert (run[f"P/{F.tag(size)}/rgba"] == oracle.colorcode(oracle.upsample_bilinear(run[f"P/{F.tag(size)}/out_low"], h, w))).all(), (case.id, size)


REFS = {}  # size -> float64 logits, made once


@gpu
@pytest.mark.parametrize("case", F.SUBFORM_CASES, ids=[c.id for c in F.SUBFORM_CASES])
def test_subform_ran_and_gives_configuration_0s_bits(shared, oracle, case):
    if F.FATAL:
        pytest.fail(f"not started: an earlier child of this module ended badly ({F.FATAL[0]})")
    base = shared.baseline(case)
    run = base if case.baseline else shared.run(case)
    try:
        check_variants(run, case)
        if case.baseline:
            if case.sizes != "edge":
                grade_baseline(run, case, oracle)
        elif case.compare == "bytes":
            check_equal(base, run, case)
        elif case.compare == "stem":
            check_equal(base, run, case, prefixes=("L/",))
            grade_product_logits(run, case, oracle, REFS)
        else:  # "layers": every layer at every size against the float64 reference, at the mode's stated bar
            assert case.sizes == "edge" and sorted(base.keys()) == sorted(run.keys())
            print(f"{case.id}: tensors that differ from the baseline's bytes: L/ {len(F.byte_differences(base, run, 'L/'))}, P/ {len(F.byte_differences(base, run, 'P/'))}")
            TF.grade_float(run, case.mode, shared.forms.float_taps(oracle), oracle, what=case.id + " ")
    finally:
        if not case.baseline:
            run.discard()
