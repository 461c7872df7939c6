"""Helper of tests/test_gpu_forms.py and tests/test_gpu_subforms.py (a plain module, no tests): the table of tile forms that are
candidates in each arithmetic mode, the table of SUB-forms (the kernels a launcher picks inside one configuration, SUBFORM_CASES), the
sizes at which every form is run, and the child process that runs ONE (mode, form, environment) over all of them.

INFUR_CONV_CFG and INFUR_HL_PIPE are read once per process (infur_tuner.cpp, conv_hl.hip), hence one child per case -- started with
subprocess.run under a time limit of its own, like tests/test_gpu_halo.py.  The child loads the model once per context and, for each
size of SIZES, writes

  L/<h>x<w>/<layer>   every conv output of a Context(keep_activations=True): the unfused launches, read back layer by layer
  L/<h>x<w>/out_low, aux_low
  P/<h>x<w>/out_low, aux_low, rgba   the product path, Context(profile=True) + FramePath.advance: the two-source conv3 + downsample
                      launch, the fused stem + pool, a reused arena -- after one frame of ANOTHER size through the same context, so
                      that stale bytes of other tensors lie behind every ragged tile

into one .npz, and the product path's (layer, kernel, variant) profile records per size into a .json next to it ("records" in its
options: also the records of the per-layer launches, with their flops and bytes, into a .records.json).  With "digest" in
its options the child keeps a SHA-1 of every array ("D/<key>") instead of the array: the forced forms of a size whose 57 layers are
1.5 GB.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w) of W.synth_frame(h, w, index=h + w), FCN-ResNet50 on the synthetic blob: the smallest sizes at which each edge still exists
SIZES = [
    (135, 241),  # stride-8 / 4 / 2 maps 17x31, 34x61, 68x121: ragged against every tile
    (97, 61),    # 13x8, 25x16, 49x31: M = 104 < every BM, partial Winograd tiles
    (128, 128),  # 16x16 = 256, 32x32 = 1024, 64x64 = 4096: M a whole number of 128- and 256-row tiles, no tail tile anywhere
    (3, 5),      # 1x1, 1x2, 2x3: maps smaller than a 16x16 halo patch and than one Winograd tile
    (1, 1),      # 1x1: M = 1
]
# the frame that goes through the product context before the measured one
PRE_FRAME = {s: (97, 61) for s in SIZES}
PRE_FRAME[(97, 61)] = (135, 241)

MODES = ("f32", "f32s", "f32x", "f16", "f16hl", "i8")

# configuration index -> kernel name as conv_igemm_config_name reports it ({t} = the mode's tag); conv_forms.h: kConvForms,
# held against this table by tests/test_conv_forms_cpu.py
_TILED = {
    0: "conv_igemm_{t}<128,128>", 1: "conv_igemm_{t}<64,128>", 2: "conv_igemm_{t}<128,64>", 3: "conv_igemm_{t}<64,64>",
    4: "conv_igemm_{t}<256,32>", 5: "conv_igemm_{t}<128,256>", 6: "conv_igemm_{t}<256,128>", 7: "conv_igemm_{t}<128,128,1buf>",
    8: "conv_igemm_{t}<128,64,1buf>", 9: "conv_igemm_{t}<64,128,1buf>", 10: "conv_igemm_{t}<64,64,1buf>",
    11: "conv_igemm_{t}<256,256,1frag>", 12: "conv_igemm_{t}<256,128,1frag>", 13: "conv_igemm_{t}<256,256,dma>",
    14: "conv_igemm_{t}<256,128,dma>", 15: "conv1x1_{t}<256,areg>", 16: "conv_igemm_{t}<256,256,dmai>",
    17: "conv_igemm_{t}<256,128,dmai>", 18: "conv1x1_{t}<256,areg,nsplit>", 19: "conv3x3_{t}<16x16,128,halo>",
    20: "conv3x3_{t}<16x16,256,halo>", 21: "conv3x3_{t}<16x16,256,halo4>",
}
# mode 5 (conv_hl.hip, conv_hl_areg.hip)
_HL = {
    0: "conv_hl<128,128>", 5: "conv_hl<128,256>", 6: "conv_hl<256,128>", 11: "conv_hl<256,256>", 12: "conv_hl<256,128,4w>",
    13: "conv_hl<256,256,wn2>", 14: "conv_hl<128,256,4w>", 15: "conv_hl<128,areg>", 16: "conv_hl<128,256,4w,wn2>",
    17: "conv_hl<256,128,4w,wn2>",
}
HL_AREG = 15  # conv_hl_areg.hip has ONE K loop: INFUR_HL_PIPE does not reach it and its name never ends in ",plain"


def _tiled(tag, cfgs):
    return {k: _TILED[k].format(t=tag) for k in cfgs}


# The configurations that are candidates for at least one layer of FCN-ResNet50 in each mode, read off conv_forms.h (ConvForm::modes)
# and the families' predicates: the register-staged tiles 0-12 everywhere; the LDS-DMA forms 13, 14, 16, 17 for byte operands that need no
# conversion (f16, i8); 15 = the 1x1 form with the activations in registers (f16, i8; 18 = its N-split, i8 only); 19 / 20 = the 3x3 form
# with the input patch in LDS (f16, i8), 21 = its four-wave form (f16 only).
FORMS = {
    "f32": _tiled("f32", range(13)),
    "f32s": _tiled("f32s", range(13)),
    "f32x": _tiled("f32x", range(13)),
    "f16": _tiled("f16", list(range(18)) + [19, 20, 21]),
    "f16hl": dict(_HL),
    "i8": _tiled("i8", range(21)),
}


def expected_kernel(mode, cfg, plain=False):
    """the profile's kernel name of a layer that runs configuration `cfg`"""
    name = FORMS[mode][cfg]
    return name + ",plain" if (mode == "f16hl" and plain and cfg != HL_AREG) else name


def cases():
    """(mode, cfg, plain) of every case: one per FORMS entry, f16hl with both K loops"""
    out = []
    for mode in MODES:
        for cfg in sorted(FORMS[mode]):
            out.append((mode, cfg, False))
            if mode == "f16hl":
                out.append((mode, cfg, True))
    return out


def tag(size):
    return f"{size[0]}x{size[1]}"


# ---- sub-forms: tests/test_gpu_subforms.py ------------------------------------------------------------------------------------------
# The smallest frame whose maps flip BOTH size rules of the f16 launchers (conv_forms.h; figures held by test_conv_forms_cpu.py):
# the stride-4 map 195 x 225 = 43,875 pixels is 172 tiles of 256 > 170 -> the 256-pixel form of configuration 15 on layer1, the
# stride-8 map 98 x 113 = 11,074 pixels (44 tiles) keeps the 128-pixel form; 98 x 113 is 56 tiles of 16 x 16: Cout 512 -> 224 > 170 ->
# N tiles of 128 in configuration 19 (layer4, the head), Cout 256 -> 112 -> N tiles of 64 (layer3).  Ragged against every tile.
NATURAL_SIZES = [(777, 897)]
# stride-8 map 8 x 32: ONE 8 x 32 tile instead of two of 16 x 16 -- the only tiling of halo_plan that FORMS' sizes never pick
# (stride-4 map 16 x 64: four tiles either way, 16 x 16 wins on its smaller patch)
GEOM_SIZES = [(64, 256)]
SIZE_SETS = {"edge": SIZES, "natural": NATURAL_SIZES, "geom": GEOM_SIZES}
for _s in NATURAL_SIZES + GEOM_SIZES:
    PRE_FRAME[_s] = (97, 61)
# the sizes that reach the edge classes the three lists above leave out: derived and held by tests/edge_cover.py (which imports this
# module: the import stands here, after everything it reads), run by tests/test_gpu_edge_cover.py
from edge_cover import COVER_SIZES  # noqa: E402

SIZE_SETS["cover"] = COVER_SIZES
for _s in COVER_SIZES:
    PRE_FRAME[_s] = (97, 61)


class SubformCase:
    """One child of tests/test_gpu_subforms.py: configuration `cfg` of `mode` under the hooks `env`, with Winograd tile `tile` (0: the
    context's default, F(6x6)), at the sizes SIZE_SETS[sizes].
    see:      variant words (conv_forms.h: kVariantWords) that must appear in the product path's profile, each a word or
              (word, layer prefix): on a layer of that prefix.
    never:    words no record may carry (the hook forces EVERY launch of the family)
    compare:  "bytes" -- every L/ and P/ array equals the baseline's bytes; "stem" (the fused stem's arithmetic differs by design) --
              the L/ arrays do (keep_activations runs the unfused stem) and the product path's logits are graded against the float64
              reference; "layers" (the transforms' roundings differ by design) -- every layer is graded against the float64 reference
    baseline: the case is the run the others of its (mode, tile, sizes) are compared with: INFUR_CONV_CFG=0 and no other hook"""

    def __init__(self, mode, cfg, env=None, tile=0, sizes="edge", see=(), never=(), compare="bytes"):
        self.mode, self.cfg, self.env, self.tile, self.sizes = mode, cfg, dict(env or {}), tile, sizes
        self.see, self.never, self.compare = tuple(see), tuple(never), compare
        assert compare in ("bytes", "stem", "layers")
        self.baseline = cfg == 0 and not self.env

    @property
    def key(self):
        """the baseline this case is compared with"""
        return (self.mode, self.tile, self.sizes)

    @property
    def id(self):
        hooks = "-".join(f"{k[6:]}={v}" for k, v in sorted(self.env.items()))
        return "-".join(x for x in (self.mode, f"cfg{self.cfg}", hooks, f"F{self.tile}" if self.tile else "", self.sizes if self.sizes != "edge" else "") if x)

    def words(self):
        return {w if isinstance(w, str) else w[0] for w in self.see}


_C = SubformCase
SUBFORM_CASES = [
    # ---- f32: the Winograd transforms (all Winograd layers have C % 128 == 0: F(6x6) runs the LDS two-pass form by default) ----
    _C("f32", 0, see=("lds", "f32stem"), never=("f32x1", "f32x2", "f32x4w")),
    _C("f32", 0, {"INFUR_WINO_LDS": "0"}, see=("f32x2",), never=("lds", "f32x1", "f32x4w")),   # per-thread F(6x6) on 128 channels and more
    # (no default dispatch reaches f32x1; its scalar expressions contract into other FMAs than the vector forms': test_gpu_subforms.py)
    _C("f32", 0, {"INFUR_WINO_VEC": "1"}, see=("f32x1",), never=("lds", "f32x2", "f32x4w"), compare="layers"),
    _C("f32", 0, {"INFUR_WINO_VEC": "2"}, see=("f32x2",), never=("lds", "f32x1", "f32x4w")),
    _C("f32", 0, tile=2, see=("f32x4w",), never=("lds", "f32x1", "f32x2")),
    _C("f32", 0, {"INFUR_WINO_VEC": "2"}, tile=2, see=("f32x2",), never=("lds", "f32x1", "f32x4w")),  # the non-vec4 F(2x2)
    _C("f32", 0, tile=4, see=("f32x4w",), never=("lds", "f32x1", "f32x2")),
    _C("f32", 0, {"INFUR_WINO_VEC": "2"}, tile=4, see=("f32x2",), never=("lds", "f32x1", "f32x4w")),  # the non-vec4 F(4x4)
    # ---- f16 ----
    _C("f16", 0, see=("f16stem",), never=("f32stem",)),
    _C("f16", 15, {"INFUR_AREG_BM": "256"}, see=("bm256",), never=("bm128",)),
    _C("f16", 19, see=("bn64", "na1", "16x16", "mixed"), never=("bn128", "bn256")),  # the size rule at small maps: N tiles of 64 everywhere
    _C("f16", 19, {"INFUR_HALO_BN": "128"}, see=("bn128", "na2", "16x16", "mixed", ("bn64", "backbone.layer1.")), never=("bn256",)),
    _C("f16", 20, see=("bn256",), never=("bn64", "bn128")),
    # the back-to-back launch: which waves issue the DMA pieces (2: the default), and the workgroup forms of INFUR_B2B_FORM
    _C("f16", 0, {"INFUR_B2B": "1", "INFUR_B2B_DMA": "0"}, see=("form3", "dma0"), never=("dma1", "dma2", "form1", "form2")),
    _C("f16", 0, {"INFUR_B2B": "1", "INFUR_B2B_DMA": "1"}, see=("form3", "dma1"), never=("dma0", "dma2", "form1", "form2")),
    _C("f16", 0, {"INFUR_B2B": "1", "INFUR_B2B_FORM": "1"}, see=("form1", "dma2"), never=("dma0", "dma1", "form2", "form3")),
    _C("f16", 0, {"INFUR_B2B": "1", "INFUR_B2B_FORM": "2"}, see=("form2", "dma2"), never=("dma0", "dma1", "form1", "form3")),
    _C("f16", 0, {"INFUR_STEM_F32": "1"}, see=("f32stem",), never=("f16stem",), compare="stem"),  # stem_pool_kernel<_Float16>
    # ---- f32s ----
    _C("f32s", 0, see=("f16stem",), never=("f32stem",)),
    _C("f32s", 0, {"INFUR_STEM_F32": "1"}, see=("f32stem",), never=("f16stem",), compare="stem"),  # the f32-MFMA stem under the split conv stack
    # ---- i8: the N split of configuration 18 (on maps this small the rule itself gives one workgroup per N tile: 2 / 4 / 8 / 16) ----
    _C("i8", 0),
    _C("i8", 18, see=("nsplit2", "nsplit4", "nsplit8", "nsplit16")),
    _C("i8", 18, {"INFUR_Q8_NSPLIT": "2"}, see=("nsplit2",), never=("nsplit4", "nsplit8", "nsplit16")),
    _C("i8", 18, {"INFUR_Q8_NSPLIT": "4"}, see=("nsplit4", ("nsplit2", "backbone.layer1.")), never=("nsplit8", "nsplit16")),  # (Cout 256: two N tiles)
    _C("i8", 18, {"INFUR_Q8_NSPLIT": "8"}, see=("nsplit8", ("nsplit4", "backbone.layer2.")), never=("nsplit16",)),
    # ---- the size rules themselves: no hook besides INFUR_CONV_CFG ----
    _C("f16", 0, sizes="natural", see=("f16stem",)),
    _C("f16", 15, sizes="natural", see=(("bm256", "backbone.layer1."), ("bm128", "backbone.layer4."))),
    _C("f16", 19, sizes="natural", see=(("bn128", "backbone.layer4."), ("bn128", "classifier."), ("bn64", "backbone.layer3."), ("bn64", "backbone.layer1."))),
    _C("f16", 0, sizes="geom", see=("f16stem",)),
    _C("f16", 19, sizes="geom", see=("8x32", ("8x32", "backbone.layer3."))),
]
del _C


def subform_baseline(case):
    for c in SUBFORM_CASES:
        if c.baseline and c.key == case.key:
            return c
    raise KeyError(case.id)


# ---- the child --------------------------------------------------------------------------------------------------------------------
def child_main(argv):
    mode, out_path, blob_path = argv[0], argv[1], argv[2]
    opts = json.loads(argv[3]) if len(argv) > 3 else {}
    sizes = [tuple(s) for s in opts.get("sizes", SIZES)]
    tile, digest = int(opts.get("tile", 0)), bool(opts.get("digest", False))
    records = bool(opts.get("records", False))  # also keep the profile of the launches that made the L/ arrays (own_error.scope_of)
    sys.path.insert(0, ROOT)
    import ctypes as C

    from infur_amd import weights as W
    from infur_amd.processors import Context, FramePath, Model, ModelCmd

    if mode == "i8":  # a quantised blob defines its own arithmetic: any context dtype
        with open(blob_path, "rb") as f:
            blob = f.read()
        dtype = "f32"
    else:
        blob = W.synth_blob()
        dtype = mode
    specs = W.graph(50)
    res = {}
    # (SIZES: the largest tensor, 128 channels of 68 x 121 in the quantised model, is half of 1 << 21; a large frame: 2048 channels of
    #  the stride-8 map, layer4's conv3 -- twice the 256 channels of the stride-4 map and four times the stem's 64 of the stride-2 one)
    buf = np.empty(max(1 << 21, max(2048 * ((h + 7) // 8 + 1) * ((w + 7) // 8 + 1) for h, w in sizes)), np.float32)

    def keep(key, a):
        if digest:
            import hashlib

            res["D/" + key] = np.frombuffer(hashlib.sha1(repr(a.shape).encode() + np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
        else:
            res[key] = a.copy()

    c = Context(device=0, dtype=dtype, keep_activations=True, profile=records, winograd_tile=tile)
    m = Model(c).control(ModelCmd.LoadBlob(blob))
    layer_records = {}
    for size in sizes:
        h, w = size
        fr = W.synth_frame(h, w, index=h + w)
        if mode == "i8":
            FramePath(c).advance(fr, 1.0)  # (as tests/test_gpu_quant.py reads its layers back)
        else:
            m.advance(fr, [])
        for i, spec in enumerate(specs):
            cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            c.check(c.L.infur_debug_read_activation(c.h, i, buf.ctypes.data, buf.size, C.byref(cc), C.byref(hh), C.byref(ww)))
            keep(f"L/{tag(size)}/{spec.name}", buf[: cc.value * hh.value * ww.value].reshape(cc.value, hh.value, ww.value))
        lo, la = m.lowres()
        keep(f"L/{tag(size)}/out_low", lo)
        keep(f"L/{tag(size)}/aux_low", la)
        if records:
            layer_records[tag(size)] = [{k: r[k] for k in ("name", "kernel", "variant", "flops", "bytes")} for r in c.profile()]
    c.close()

    kernels = {}
    c = Context(device=0, dtype=dtype, profile=True, winograd_tile=tile)
    m = Model(c).control(ModelCmd.LoadBlob(blob))
    fp = FramePath(c)
    for size in sizes:
        h, w = size
        ph, pw = PRE_FRAME[size]
        fp.advance(W.synth_frame(ph, pw, index=7), 1.0)
        rgba, _ = fp.advance(W.synth_frame(h, w, index=h + w), 1.0)
        lo, la = m.lowres()
        keep(f"P/{tag(size)}/out_low", lo)
        keep(f"P/{tag(size)}/aux_low", la)
        keep(f"P/{tag(size)}/rgba", rgba)
        kernels[tag(size)] = [[r["name"], r["kernel"], r["variant"]] for r in c.profile()]
    c.close()

    np.savez(out_path, **res)
    with open(out_path + ".json", "w") as f:
        json.dump(kernels, f)
    if records:
        with open(out_path + ".records.json", "w") as f:
            json.dump(layer_records, f)
    print("FORMS CHILD OK")


# ---- the parent -------------------------------------------------------------------------------------------------------------------
# One model load per context plus fifteen tiny frames, the read-back of 5 x 57 layers and the .npz: 3 s per child measured on an
# MI355X, 6 s for the first child of a run (cold caches); the limit is five times that.
CHILD_TIMEOUT = 30

# Set by the first child that ends by a signal, an abort or its time limit, or that reports a GPU memory fault: nothing more is
# started on the GPU by this module after that (a faulted card is left alone; there are no retries anywhere in here).
FATAL = []
_FATAL_CODES = (134, 139, 124, 137)
_FATAL_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")


# every hook that selects a sub-form (each is read once per process into a static, hence one child per case)
SUBFORM_HOOKS = ("INFUR_AREG_BM", "INFUR_Q8_NSPLIT", "INFUR_HALO_BN", "INFUR_WINO_LDS", "INFUR_WINO_VEC", "INFUR_B2B", "INFUR_B2B_DMA",
                 "INFUR_B2B_FORM", "INFUR_STEM_F32")


class ChildFailed(AssertionError):
    pass


class Run:
    """what one child left: the arrays (loaded on demand) and the product path's profile per size"""

    def __init__(self, path):
        self.path = path
        self.npz = np.load(path)
        with open(path + ".json") as f:
            recs = json.load(f)
        self.kernels = {k: [(r[0], r[1]) for r in v] for k, v in recs.items()}  # size -> (layer, kernel)
        self.variants = {k: [tuple(r) for r in v] for k, v in recs.items()}  # size -> (layer, kernel, variant)
        self.layer_records = None  # size -> the per-layer launches' records (a child run with records=True)
        if os.path.exists(path + ".records.json"):
            with open(path + ".records.json") as f:
                self.layer_records = json.load(f)

    def keys(self):
        return self.npz.files

    def __getitem__(self, k):
        return self.npz[k]

    def discard(self):
        """the arrays of a form that has been compared are not needed again"""
        self.npz.close()
        for p in (self.path, self.path + ".json", self.path + ".records.json"):
            if os.path.exists(p):
                os.remove(p)


def run_child(mode, cfg, plain, out_path, qblob_path="", extra_env=None, tile=0, sizes=None, digest=False, timeout=None, records=False):
    """One child process for (mode, cfg, K loop) -> Run.  Raises ChildFailed; sets FATAL when the way the child ended says the GPU
    may be in trouble.  extra_env: hooks besides INFUR_CONV_CFG / INFUR_HL_PIPE; tile: the contexts' Winograd tile (0: default);
    sizes: instead of SIZES; digest: keep a digest of every array instead of the array; timeout: instead of CHILD_TIMEOUT; records:
    the profile of the per-layer launches too (Run.layer_records)."""
    timeout = timeout or CHILD_TIMEOUT
    if FATAL:
        raise ChildFailed(f"not started: an earlier child of this module ended badly ({FATAL[0]})")
    env = dict(os.environ)
    env["INFUR_CONV_CFG"] = str(cfg)
    env.pop("INFUR_HL_PIPE", None)
    if plain:
        env["INFUR_HL_PIPE"] = "0"
    for k in SUBFORM_HOOKS:  # (a hook of the caller's environment is no part of any case)
        env.pop(k, None)
    env.update(extra_env or {})
    what = f"{mode} cfg {cfg}{' plain' if plain else ''}" + "".join(f" {k}={v}" for k, v in sorted((extra_env or {}).items())) + \
           (f" F({tile}x{tile})" if tile else "") + (f" at {[tag(s) for s in sizes]}" if sizes else "")
    opts = {"tile": tile, "digest": digest}
    if records:
        opts["records"] = True
    if sizes:
        opts["sizes"] = [list(s) for s in sizes]
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out_path, qblob_path, json.dumps(opts)], env=env, timeout=timeout,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        FATAL.append(f"{what}: no result after {timeout} s")
        raise ChildFailed(FATAL[0])
    log = r.stdout[-3000:] + r.stderr[-3000:]
    if r.returncode < 0 or r.returncode in _FATAL_CODES or any(t in r.stdout or t in r.stderr for t in _FATAL_TEXT):
        FATAL.append(f"{what}: return code {r.returncode}")
        raise ChildFailed(FATAL[0] + "\n" + log)
    if r.returncode != 0 or "FORMS CHILD OK" not in r.stdout:
        raise ChildFailed(f"{what}: return code {r.returncode}\n{log}")
    return Run(out_path)


def digests(run):
    """key -> digest of the array's bytes (and shape): what is kept of a run whose arrays are discarded"""
    import hashlib

    return {k: hashlib.sha1(repr(run[k].shape).encode() + np.ascontiguousarray(run[k]).tobytes()).hexdigest() for k in run.keys()}


def byte_differences(ref, got, prefix):
    """keys under `prefix` whose bytes differ between two runs -> [(key, number of differing elements)]"""
    bad = []
    for k in ref.keys():
        if not k.startswith(prefix):
            continue
        a, b = ref[k], got[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append((k, -1))
        elif not (a.view(np.uint8) == b.view(np.uint8)).all():
            bad.append((k, int((a.view(np.uint8).reshape(-1, a.itemsize) != b.view(np.uint8).reshape(-1, a.itemsize)).any(-1).sum())))
    return bad


if __name__ == "__main__":
    child_main(sys.argv[1:])
