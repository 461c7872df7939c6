"""Helper of tests/test_gpu_forms.py (a plain module, no tests): the table of tile forms that are candidates in each arithmetic mode,
the sizes at which every form is run, and the child process that runs ONE (mode, form, environment) over all of them.

INFUR_CONV_CFG and INFUR_HL_PIPE are read once per process (infur_tuner.cpp, conv_hl.hip), hence one child per case -- started with
subprocess.run under a time limit of its own, like tests/test_gpu_halo.py.  The child loads the model once per context and, for each
size of SIZES, writes

  L/<h>x<w>/<layer>   every conv output of a Context(keep_activations=True): the unfused launches, read back layer by layer
  L/<h>x<w>/out_low, aux_low
  P/<h>x<w>/out_low, aux_low, rgba   the product path, Context(profile=True) + FramePath.advance: the two-source conv3 + downsample
                      launch, the fused stem + pool, a reused arena -- after one frame of ANOTHER size through the same context, so
                      that stale bytes of other tensors lie behind every ragged tile

into one .npz, and the product path's (layer, kernel) profile records per size into a .json next to it.
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


# ---- the child --------------------------------------------------------------------------------------------------------------------
def child_main(argv):
    mode, out_path, blob_path = argv[0], argv[1], argv[2]
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
    buf = np.empty(1 << 21, np.float32)  # (the largest tensor, 128 channels of 68 x 121 in the quantised model, is half of it)

    c = Context(device=0, dtype=dtype, keep_activations=True)
    m = Model(c).control(ModelCmd.LoadBlob(blob))
    for size in SIZES:
        h, w = size
        fr = W.synth_frame(h, w, index=h + w)
        if mode == "i8":
            FramePath(c).advance(fr, 1.0)  # (as tests/test_gpu_quant.py reads its layers back)
        else:
            m.advance(fr, [])
        for i, spec in enumerate(specs):
            cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            c.check(c.L.infur_debug_read_activation(c.h, i, buf.ctypes.data, buf.size, C.byref(cc), C.byref(hh), C.byref(ww)))
            res[f"L/{tag(size)}/{spec.name}"] = buf[: cc.value * hh.value * ww.value].reshape(cc.value, hh.value, ww.value).copy()
        lo, la = m.lowres()
        res[f"L/{tag(size)}/out_low"], res[f"L/{tag(size)}/aux_low"] = lo.copy(), la.copy()
    c.close()

    kernels = {}
    c = Context(device=0, dtype=dtype, profile=True)
    m = Model(c).control(ModelCmd.LoadBlob(blob))
    fp = FramePath(c)
    for size in SIZES:
        h, w = size
        ph, pw = PRE_FRAME[size]
        fp.advance(W.synth_frame(ph, pw, index=7), 1.0)
        rgba, _ = fp.advance(W.synth_frame(h, w, index=h + w), 1.0)
        lo, la = m.lowres()
        res[f"P/{tag(size)}/out_low"], res[f"P/{tag(size)}/aux_low"], res[f"P/{tag(size)}/rgba"] = lo.copy(), la.copy(), rgba.copy()
        kernels[tag(size)] = [[r["name"], r["kernel"]] for r in c.profile()]
    c.close()

    np.savez(out_path, **res)
    with open(out_path + ".json", "w") as f:
        json.dump(kernels, f)
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


class ChildFailed(AssertionError):
    pass


class Run:
    """what one child left: the arrays (loaded on demand) and the product path's profile per size"""

    def __init__(self, path):
        self.path = path
        self.npz = np.load(path)
        with open(path + ".json") as f:
            self.kernels = {k: [tuple(r) for r in v] for k, v in json.load(f).items()}

    def keys(self):
        return self.npz.files

    def __getitem__(self, k):
        return self.npz[k]

    def discard(self):
        """the arrays of a form that has been compared are not needed again"""
        self.npz.close()
        for p in (self.path, self.path + ".json"):
            if os.path.exists(p):
                os.remove(p)


def run_child(mode, cfg, plain, out_path, qblob_path=""):
    """One child process for (mode, cfg, K loop) -> Run.  Raises ChildFailed; sets FATAL when the way the child ended says the GPU
    may be in trouble."""
    if FATAL:
        raise ChildFailed(f"not started: an earlier child of this module ended badly ({FATAL[0]})")
    env = dict(os.environ)
    env["INFUR_CONV_CFG"] = str(cfg)
    env.pop("INFUR_HL_PIPE", None)
    if plain:
        env["INFUR_HL_PIPE"] = "0"
    what = f"{mode} cfg {cfg}{' plain' if plain else ''}"
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out_path, qblob_path], env=env, timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        FATAL.append(f"{what}: no result after {CHILD_TIMEOUT} s")
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
