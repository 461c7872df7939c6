"""Each conv layer graded ALONE: the device's output of layer i against a float64 evaluation of layer i on the inputs the device
itself stored ("teacher forcing", TorchModel.forward_lowres(forced=...)).  The error the chain accumulated upstream cancels; what is
left is the kernel's own arithmetic (measured: LAB_NOTES.md, "each conv layer graded alone"; the own/* rows of tests/accuracy.py).  A plain helper
module like tests/accuracy.py: no tests, no fixtures (tests/test_gpu_own_error.py, tests/test_own_error_cpu.py).

  read_all(ctx, depth, hw)                       -> {name: f32 [C,H,W]}: every kept activation, shapes held against weights.plan
  grade_own(ctx, model64, chw, mode, variant, where) -> the table: one row per layer (name, scope, kernel, four readings, misses)

The scope of a layer comes from WHAT RAN -- the kernel names of the layer's records in Context.profile() -- never from the options:
  own/1x1                1x1 convs: the bottlenecks' conv1 / conv3, the downsample branches, both halves of a fused conv3 + next conv1 launch
  own/direct             k > 1 convs on a direct / implicit-GEMM / halo kernel, and the stem
  own/wino2, 4, 6        the layer's records name the Winograd transforms; the tile is the one whose (tile + 2)^2 planes and tile count
                         the batched GEMM's record executed (its `flops` and `bytes`: scope_of)
  own/head               classifier.4 / aux_classifier.4: f32 output in every mode
  own16/<kind>           f16 mode only, second grading: the reference's conv weights rounded to f16 first (exact arithmetic on the
                         operands the kernel held: what remains is the f32 accumulation and ONE rounding of the output)

What the code says about the two things this grading leans on (read, not assumed):

Is the read-back exact?  infur_debug_read_activation converts on the device and copies f32.  f32 tensors: a copy.  f16 tensors
(launch_nhwc_to_planar): f16 -> f32, exact.  Three-byte tensors (hl_tensor.hip: hl_nhwc_to_planar_kernel): (float)hi + bf8(lo) * kHlLoInv
in f32, kHlLoInv = 1 / (2048 x 1.09) rounded to f32 -- NOT exact: the product is rounded (or fused into the sum) and the sum is rounded
once.  |lo / kHlLoScale| <= 2^-11 |hi| (half an f16 ulp), so the constant's and the product's roundings are <= 2^-24 x 2^-11 |x| each and
the sum's <= 2^-24 |x|: the read-back is within 2^-24 (1 + 2^-10) |x| ~ 6.0e-8 |x| of the stored value, three orders below the f16hl
own error measured here.  The consumers divide kHlDebias out in their own arithmetic (hl_lo8_to_f32, the bf8 MFMA's block scale):
that is the consumer's own error and is graded as such.

Does the device round between a kept tensor and its consumer's input?  Once.  Under keep_activations the stem and the max-pool run
unfused (infur_capi.cpp: forward).  f32 / f32s / f32x keep f32 and pool in f32, f16 keeps f16 and pools in f16 (a maximum: exact).
f16hl keeps the stem's output as F32 (the exact f32 stem), pools in f32 and only THEN converts the pooled tensor to hi / lo planes
(launch_hl_from_f32: <= 2^-14 per element).  The forced walk feeds the pool of the kept f32 tensor, so that one conversion lands in the
readings of the pool's two consumers, HL_STEM_FED.  They are graded by their scope's bars like every layer; the other layers of the
scope are NOT given room for them: where the two stand above the rest, the rest gets the tighter HL_REST_CAP.

The f16 mode's weights: repack_oihw_to_ohwi_kernel<_Float16> is `(T)src[...]`, a v_cvt_f16_f32 under the default rounding mode, round
to nearest even with subnormals: numpy's astype(np.float16) is its host twin.  The stem is the exception: launch_repack_stem keeps f32
and stem_conv7x7_kernel multiplies in f32 in every mode, so the own16 reference leaves the stem's weights alone.  Biases stay f32.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402

from infur_amd import weights as W  # noqa: E402

KINDS = ("1x1", "direct", "wino2", "wino4", "wino6", "head")
OWN_SCOPES = ("own/1x1", "own/direct", "own/wino2", "own/wino4", "own/wino6", "own/head")
OWN16_SCOPES = ("own16/1x1", "own16/direct", "own16/head")
assert OWN_SCOPES == tuple("own/" + k for k in KINDS)

# f16hl: the consumers of the pooled stem tensor, whose input the device converted to three bytes after the kept tensor was taken
HL_STEM_FED = ("backbone.layer1.0.conv1", "backbone.layer1.0.downsample.0")
# f16hl: tighter bars (max_rel, elem, rms, bias) for the layers of a scope OTHER than HL_STEM_FED, 1.3 x their own worst -- only where
# the two stand above them.  Measured: they do not (LAB_NOTES.md, "Own error"): no entry.
HL_REST_CAP = {}


# ---- what ran ----------------------------------------------------------------------------------------------------------------------
def kernel_kind(kernel):
    """the family of a profile record's kernel name (conv_forms.h: conv_family_prefix, infur_capi.cpp's ProfScopes); a name this
    module does not know is an error, not a guess"""
    if kernel in ("wino_input", "wino_output", "wino_input_hl", "wino_output_hl"):
        return "wino"
    if kernel in ("stem_conv7x7", "stem_pool"):
        return "stem"
    if kernel == "conv1x1_b2b_f16":
        return "b2b"
    form = kernel[: -len(",plain")] if kernel.startswith("conv_hl<") and kernel.endswith(">,plain") else kernel  # (INFUR_HL_PIPE=0)
    if form.startswith(("conv_igemm_", "conv1x1_", "conv3x3_", "conv_hl<")) and form.endswith(">") and "?" not in form:
        return "gemm"
    raise ValueError(f"own_error: unknown kernel name {kernel!r}")


def layer_records(records, specs):
    """{conv name: [records of the launches that produced it]} from Context.profile().  A record is named after its layer, with
    "/in" / "/out" for the Winograd transforms and "+..." where one launch does more (conv3 + the next block's conv1, the stem + pool)"""
    names = [s.name for s in specs]
    out = {n: [] for n in names}
    for r in records:
        base, _, rest = r["name"].partition("+")
        for suffix in ("/in", "/out"):
            if base.endswith(suffix):
                base = base[: -len(suffix)]
        if base not in out:
            continue  # the max-pool, the pre- and post-processing stages
        out[base].append(r)
        if rest == "next.conv1":
            i = names.index(base) + 1
            while specs[i].role != "conv1":
                i += 1
            out[names[i]].append(r)
        elif rest == "downsample":
            out[names[names.index(base) + 1]].append(r)
        elif rest not in ("", "maxpool"):
            raise ValueError(f"own_error: unknown record name {r['name']!r}")
    return out


def wino_tiles(h, w, d, mt):
    """winograd.hip: wino_num_tiles"""
    return d * d * (((h + d - 1) // d + mt - 1) // mt) * (((w + d - 1) // d + mt - 1) // mt)


def scope_of(spec, recs, hw):
    """-> (own/<kind>, the kernel names) of one layer from the records of its launches; hw: the layer's output size"""
    if not recs:
        raise ValueError(f"own_error: no profile record for {spec.name}")
    kinds = [kernel_kind(r["kernel"]) for r in recs]
    kernels = "+".join(r["kernel"] for r in recs)
    if spec.role in ("cls", "auxcls"):
        assert kinds == ["gemm"], (spec.name, kernels)
        return "own/head", kernels
    if "wino" in kinds:
        gemm = [r for r, k in zip(recs, kinds) if k == "gemm"]
        assert sorted(kinds) == ["gemm", "wino", "wino"] and spec.k == 3 and spec.stride == 1, (spec.name, kernels)
        # the batched GEMM's record (infur_capi.cpp: run_conv): flops = 2 P T Cout Cin, bytes = P T (Cin es + 4 Cout) + P Cout Cin es with
        # P = (tile + 2)^2 planes of T tiles, es = 4 bytes (3: hi / lo planes).  P T alone is ambiguous (13 x 8, dilation 2: F(2x2) and
        # F(6x6) both give 512); the weight term holds P by itself
        es = 3 if any(r["kernel"].endswith("_hl") for r in recs) else 4
        pt = gemm[0]["flops"] / (2.0 * spec.cout * spec.cin)
        planes = (gemm[0]["bytes"] - pt * (spec.cin * es + 4 * spec.cout)) / (spec.cout * spec.cin * es)
        tiles = [mt for mt in (2, 4, 6) if planes == (mt + 2) ** 2 and pt == planes * wino_tiles(hw[0], hw[1], spec.dil, mt)]
        if len(tiles) != 1:
            raise ValueError(f"own_error: {spec.name}: a Winograd GEMM of {pt:g} plane tiles in {planes:g} planes is no tile's at {hw}")
        return f"own/wino{tiles[0]}", kernels
    if spec.k == 1:
        assert len(recs) == 1 and kinds[0] in ("gemm", "b2b"), (spec.name, kernels)
        return "own/1x1", kernels
    assert len(recs) == 1 and kinds[0] == ("stem" if spec.role == "stem" else "gemm"), (spec.name, kernels)
    return "own/direct", kernels


# ---- the device's tensors ------------------------------------------------------------------------------------------------------------
def read_all(ctx, depth, hw):
    """every conv output of the context's last frame (keep_activations), blob order -> {name: f32 array [C,H,W]}; hw: the frame's size"""
    plan = W.plan(hw[0], hw[1], depth)
    buf = np.empty(max(c.cout * oh * ow for c, _, _, oh, ow in plan), np.float32)
    out = {}
    for i, (spec, _, _, oh, ow) in enumerate(plan):
        cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        ctx.check(ctx.L.infur_debug_read_activation(ctx.h, i, buf.ctypes.data, buf.size, C.byref(cc), C.byref(hh), C.byref(ww)))
        assert (cc.value, hh.value, ww.value) == (spec.cout, oh, ow), (spec.name, cc.value, hh.value, ww.value)
        out[spec.name] = buf[: spec.cout * oh * ow].reshape(spec.cout, oh, ow).copy()
    return out


def forced_taps(model, chw, acts):
    """{name: float64 array}: every layer of `model` evaluated alone on the tensors of `acts`"""
    missing = [s.name for s in model.specs if s.name not in acts]
    assert not missing, missing  # (a conv without an entry would hand on its own result: no longer one layer alone)
    taps = {}
    model.forward_lowres(chw, taps=taps, forced=acts)
    return {k: v.numpy() for k, v in taps.items()}


def f16_weight_model(model64):
    """the float64 model with every conv's weights rounded to f16 as the f16 mode's repack does (module docstring); the stem's stay"""
    import copy

    m = copy.copy(model64)
    m.params = [(w if s.role == "stem" else w.float().half().double(), b) for s, (w, b) in zip(model64.specs, model64.params)]
    return m


def grade_rows(acts, taps64, records, specs, mode, where, taps16=None):
    """one row per layer: dict(name, scope, kernel, r, bad[, r16, bad16]).  Nothing is asserted here: the caller prints the table
    first (format_table) and then holds it (assert_table)."""
    by_layer = layer_records(records, specs)
    rows = []
    for spec in specs:
        got = acts[spec.name]
        scope, kernels = scope_of(spec, by_layer[spec.name], got.shape[1:])
        cap = HL_REST_CAP.get(scope) if mode == "f16hl" and spec.name not in HL_STEM_FED else None
        r = A.grade(got, taps64[spec.name], mode, scope, f"{where} {spec.name}", cap=cap, check=False)
        row = {"name": spec.name, "scope": scope, "kernel": kernels, "r": r, "bad": A.failures(r, mode, scope, cap), "mode": mode, "cap": cap}
        if taps16 is not None:
            s16 = scope.replace("own/", "own16/")
            row["r16"] = A.grade(got, taps16[spec.name], mode, s16, f"{where} {spec.name}", check=False)
            row["bad16"] = A.failures(row["r16"], mode, s16)
        rows.append(row)
    return rows


def grade_own(ctx, model64, chw, mode, variant, where, model16=None):
    """The context's last frame, layer by layer, on its own arithmetic -> the table (grade_rows).  ctx: Context(keep_activations=True,
    profile=True) after one advance of the frame whose normalised planes are `chw`; model64: TorchModel(blob, float64=True) of the same
    blob; model16 (f16 mode): f16_weight_model(model64) for the second grading."""
    depth = model64.meta["depth"]
    acts = read_all(ctx, depth, chw.shape[1:])
    taps64 = forced_taps(model64, chw, acts)
    taps16 = forced_taps(model16, chw, acts) if model16 is not None else None
    return grade_rows(acts, taps64, ctx.profile(), model64.specs, mode, f"{where} {variant}", taps16)


def format_table(rows, title):
    out = [f"{title}: per layer (max_rel, elem, rms, bias) against the float64 evaluation of that layer on the device's own inputs"]
    for row in rows:
        line = f"   {row['name']:34s} {row['scope']:11s} " + " ".join(f"{x:.2e}" for x in row["r"])
        if "r16" in row:
            line += "  | f16 weights: " + " ".join(f"{x:.2e}" for x in row["r16"])
        out.append(line + f"  {row['kernel']}" + ("".join(f"  MISSES {n}" for n in row["bad"] + [n + "(own16)" for n in row.get("bad16", [])])))
    return "\n".join(out)


def assert_table(rows):
    bad = [A.message(row["r"], row["mode"], row["scope"], row["name"], row["cap"], row["bad"]) for row in rows if row["bad"]]
    bad += [A.message(row["r16"], row["mode"], row["scope"].replace("own/", "own16/"), row["name"], None, row["bad16"]) for row in rows if row.get("bad16")]
    assert not bad, "\n".join(bad)


# ---- three planted faults: host arithmetic on read-back tensors (tests/test_gpu_own_error.py, tests/test_own_error_cpu.py) ------------
Q1_LAYER, Q1_INPUT = "backbone.layer3.0.conv2", "backbone.layer3.0.conv1"
# The kernel row whose taps output row 0 loses.  Row 0 of a pad-1 3x3 conv meets ky = 0 on the PADDING only: dropping those taps changes
# no bit (held by tests/test_own_error_cpu.py), so the plant drops the first kernel row that meets data there.
Q1_KY = 1
Q2_LAYER = "backbone.layer2.1.conv3"
Q3_LAYER, Q3_INPUT, Q3_RESIDUAL = "backbone.layer4.0.conv3", "backbone.layer4.0.conv2", "backbone.layer4.0.downsample.0"


def params_of(blob):
    """{conv name: (weights float64 [O,I,k,k], bias float64 [O])} of a blob"""
    _, tensors = W.unpack_blob(blob)
    return {name: (np.array(w, np.float64), np.array(b, np.float64)) for name, w, b in tensors}


def conv64(x, w, b, spec):
    """one conv of the graph in float64 (bias, no residual, no ReLU): x [Cin,H,W] -> [Cout,OH,OW]"""
    import torch

    y = torch.nn.functional.conv2d(torch.from_numpy(np.asarray(x, np.float64))[None], torch.from_numpy(w), torch.from_numpy(b), stride=spec.stride,
                                   padding=spec.pad, dilation=spec.dil)
    return y[0].numpy()


def plant_q1(acts, params, specs, ky=Q1_KY):
    """Q1, a dropped tap row on a border: Q1_LAYER's output with output row 0 recomputed in float64 from the input the device stored,
    WITHOUT the taps of kernel row `ky`; every other row stays the device's"""
    spec, = [s for s in specs if s.name == Q1_LAYER]
    w, b = params[Q1_LAYER]
    w = w.copy()
    w[:, :, ky, :] = 0.0
    out = np.array(acts[Q1_LAYER], np.float64)
    out[:, 0, :] = np.maximum(conv64(acts[Q1_INPUT], w, b, spec), 0.0)[:, 0, :]
    return out


def plant_q2(ref64):
    """Q2, truncation where the kernel rounds: the float64 reference of a layer cut toward zero to f16"""
    ref64 = np.asarray(ref64, np.float64)
    h = ref64.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(ref64)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(np.float64)


def plant_q3(acts, params):
    """Q3, accuracy.plant_p2 on a mid-network 1x1: the last M mod 128 pixels of Q3_LAYER's output recomputed in float64 (bias, the
    downsample branch's tensor, ReLU) from the inputs the device stored, without input channels 480..511"""
    w, b = params[Q3_LAYER]
    w = w.reshape(w.shape[0], w.shape[1])
    x, idt = np.asarray(acts[Q3_INPUT], np.float64), np.asarray(acts[Q3_RESIDUAL], np.float64)
    out = np.array(acts[Q3_LAYER], np.float64)
    k, hh, ww = out.shape
    tail = (hh * ww) % A.TAIL_TILE
    assert tail > 0 and x.shape[0] == 512
    xs = x.reshape(512, hh * ww)[:, -tail:].copy()
    xs[A.MISSED_K] = 0.0
    out.reshape(k, hh * ww)[:, -tail:] = np.maximum(w @ xs + b[:, None] + idt.reshape(k, hh * ww)[:, -tail:], 0.0)
    return out
