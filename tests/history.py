"""Helper of tests/test_gpu_history.py and tests/test_history_cpu.py (a plain module, no tests, no GPU code at import time): the
frames a context is walked through before it runs a TARGET frame, and the comparison of what it then computes.

What a context computes for a frame must depend on the model, the options and that frame only.  The runtime makes the opposite
easy: the activation pool (pool_acquire, infur_capi.cpp) hands out any free buffer that is large enough and is never cleared, it
survives a model reload, the three-byte mode's lo plane moves with the tensor's size, the staging buffers only grow, and several
kernels get their edges right by reading first and masking afterwards.  So every target below is run after frames that leave
the worst bytes behind it:

  BIG    larger than the target in every tensor: valid-looking values directly behind the last element of each tensor
  NEAR   (h+2, w+2): some tensors one row / column larger, the others exactly the target's
  SAME   the target's size, other content: stale data in exactly the target's layout (an element nobody writes keeps it)
  LOUD   BIG through a model whose stem is 10^4 times louder: Inf in the f16 mode, the 65520 clamp in f16hl, large f32 elsewhere

All of them come from the library's own earlier frames, through the public API.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from infur_amd import weights as W  # noqa: E402

MODES = ["f32", "f32s", "f32x", "f16", "f16hl", "i8"]  # i8: Context(dtype="f32") + the quantised blob, which defines its own arithmetic

# (h, w): ragged against every tile, the smallest sizes at which each edge still exists
TARGETS = [
    (75, 109),  # stem 38x55, pooled 19x28, low-res 10x14: partial F(2x2) / F(4x4) / F(6x6) tiles, unequal dilation-4 sub-grids
    (66, 130),  # pooled 17x33, low-res 9x17: odd everywhere behind an even frame
    (17, 33),   # pooled 5x9, low-res 3x5: smaller than one F(6x6) tile, M < every BM
    (5, 7),     # pooled 2x2, low-res 1x1
    (1, 1),     # 1-pixel maps
]
FULL_TARGET = (75, 109)  # the target whose walk also reads the full-resolution planes of Model.advance
BIG = (136, 248)
LOUD_GAIN = 1.0e4

# W.synth_frame indices: a target uses h + w (196 at most), the poison frames these
IDX_BIG, IDX_NEAR, IDX_SAME, IDX_LOUD = 1001, 1002, 1003, 1004

POOL_TRIM_AFTER = 4  # infur_rt.h: kPoolTrimAfter -- the pool is trimmed at the frame that many same-size frames follow the first


def target_index(size):
    return size[0] + size[1]


def near_sizes(target):
    """The NEAR frames of a target: (h+2, w+2).  From (5, 7) that frame is larger in EVERY tensor (stem 4x5 / 3x4, pooled 2x3 / 2x2,
    low-res 1x2 / 1x1) -- a second BIG; there (h+2, w+1) follows it, whose pooled map and everything behind it are the target's."""
    h, w = target
    first = (h + 2, w + 2)
    if any(a == b for a, b in zip(tensor_elems(first), tensor_elems(target))):
        return [first]
    return [first, (h + 2, w + 1)]


def tensor_elems(size):
    """oh * ow * cout of every conv of the graph at this frame size"""
    return [oh * ow * spec.cout for spec, _, _, oh, ow in W.plan(size[0], size[1])]


def stem_gain_blob(gain):
    """the synthetic parameters with the stem's weights and bias x gain: every activation behind the stem scales with it"""
    tensors = [(s, w * np.float32(gain), b * np.float32(gain)) if s.name == "backbone.conv1" else (s, w, b)
               for s, w, b in W.synth_tensors(depth=50)]
    return W.pack_blob(tensors, 50, W.NUM_CLASSES, True)


def walk_steps(target, loud=True):
    """The forwards of walk(), in order: (what, (h, w), frame index, model, forwards).  `forwards` is how many network forwards the
    step costs -- two where the full-resolution planes are read as well (FramePath.advance, then Model.advance)."""
    full = target == FULL_TARGET
    ti = target_index(target)
    steps = [("poison", BIG, IDX_BIG, "normal", 1), ("target", target, ti, "normal", 2 if full else 1)]
    for k, near in enumerate(near_sizes(target)):
        steps += [("poison", near, IDX_NEAR + 10 * k, "normal", 1), ("target", target, ti, "normal", 1)]
    steps += [("poison", target, IDX_SAME, "normal", 1), ("target", target, ti, "normal", 1)]
    # (no loud model in i8: the quantised blob clamps to u8 whatever the stem does; BIG goes through the normal one again)
    steps += [("poison", BIG, IDX_LOUD, "loud" if loud else "normal", 1), ("target", target, ti, "normal", 2 if full else 1)]
    return steps


def forward_sizes(steps):
    """the frame size of every network forward of a walk, in order"""
    out = []
    for _, size, _, _, n in steps:
        out += [size] * n
    return out


def longest_equal_run(seq):
    best = run = 0
    prev = object()
    for s in seq:
        run = run + 1 if s == prev else 1
        prev = s
        best = max(best, run)
    return best


# ---- running (GPU; everything below takes a live Context) --------------------------------------------------------------------------
def context(mode, **kw):
    from infur_amd.processors import Context

    return Context(device=0, dtype="f32" if mode == "i8" else mode, **kw)


def load(ctx, blob):
    from infur_amd.processors import Model, ModelCmd

    return Model(ctx).control(ModelCmd.LoadBlob(blob))


def run(ctx, model, frame, factor=1.0, want_scaled=False, full=False, scale_mode=0):
    """One frame through the product path -> {key: array}: `lo` / `la` the low-res logits, `rgba` the mask, `scaled` the scaled
    frame when asked, `out` / `aux` the full-resolution planes of Model.advance when asked (a second forward of the same frame)."""
    from infur_amd.processors import FramePath

    rgba, scaled = FramePath(ctx, scale_mode).advance(frame, factor, want_scaled=want_scaled)
    lo, la = model.lowres()
    res = {"lo": lo.copy(), "la": la.copy(), "rgba": rgba.copy()}
    if want_scaled:
        res["scaled"] = scaled.copy()
    if full:
        planes = []
        model.advance(frame, planes)
        res["out"], res["aux"] = planes[0], planes[1]
        lo2, la2 = model.lowres()
        res["lo_full"], res["la_full"] = lo2.copy(), la2.copy()
    return res


def kept_layers(ctx):
    """every tensor of a keep_activations context after a frame: {conv name: [c, h, w] f32 as infur_debug_read_activation gives it}"""
    import ctypes as C

    out = {}
    buf = None
    for i, spec in enumerate(W.graph(50)):
        cc, hh, ww = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if buf is None:
            buf = np.empty(1 << 21, np.float32)
        ctx.check(ctx.L.infur_debug_read_activation(ctx.h, i, buf.ctypes.data, buf.size, C.byref(cc), C.byref(hh), C.byref(ww)))
        out[spec.name] = buf[: cc.value * hh.value * ww.value].reshape(cc.value, hh.value, ww.value).copy()
    return out


def first_difference(a, b):
    """None when two results are the same bytes; otherwise a sentence naming the first key (in a's order), the number of elements
    that differ, the first index and the two values there."""
    for k in a:
        if k not in b:
            return f"{k}: missing on one side"
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        ne = (x.view(np.uint8).reshape(-1, x.itemsize) != y.view(np.uint8).reshape(-1, x.itemsize)).any(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0])
            idx = tuple(int(v) for v in np.unravel_index(i, x.shape))
            return f"{k}: {int(ne.sum())} of {ne.size} elements differ, first at {idx}: {x.reshape(-1)[i]!r} against {y.reshape(-1)[i]!r}"
    extra = [k for k in b if k not in a]
    return f"{extra[0]}: missing on one side" if extra else None


def walk(ctx, model, target, normal_blob, loud_blob):
    """BIG -> target; NEAR -> target; SAME -> target; load loud, BIG, reload normal -> target (walk_steps): the target's results,
    in order.  A poison frame's own output is not looked at beyond the call returning OK.  Size changes reset the runtime's
    same-size count, so the pool is never trimmed and every stale buffer stays in it."""
    from infur_amd.processors import FramePath, ModelCmd

    fp = FramePath(ctx)
    results = []
    loaded = "normal"
    for what, size, index, which, forwards in walk_steps(target, loud=loud_blob is not None):
        if which != loaded:
            model.control(ModelCmd.LoadBlob(loud_blob if which == "loud" else normal_blob))
            loaded = which
        frame = W.synth_frame(size[0], size[1], index=index)
        if what == "poison":
            fp.advance(frame, 1.0)
        else:
            results.append(run(ctx, model, frame, full=forwards == 2))
    return results
