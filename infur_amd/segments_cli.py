"""Headless segmentation front end: packed bgr24 frames in, class planes and one caption record line per frame out.

    ffmpeg -i in.mp4 -an -f image2pipe -pix_fmt bgr24 -c:v rawvideo pipe:1 \
      | python -m infur_amd.segments_cli --width 1280 --height 720 --scale 0.5 --model fcn.infurw \
            --labels-out labels.u8 --stats-out captions.jsonl --softmax

``--labels-out`` receives the argmax class planes back to back (ow*oh bytes per frame, one byte per pixel);
``--stats-out`` one JSON line per frame: ``{"frame": n, "width": ow, "height": oh, "classes": [class_summary records]}``
(name, pixels, share, centroid, box, mean confidence of every class that occurs -- the "class label captions" of the
reference's todo list).  ``--softmax`` decodes logits with the softmax probability as confidence instead of the
reference's raw ``c_max * 255``.  Frames go through the fused scale -> model -> segments path one at a time.
"""
from __future__ import annotations

import argparse
import json
import sys
import time


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--width", type=int, required=True)
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--bilinear", action="store_true", help="bilinear Scale instead of the reference's nearest")
    ap.add_argument("--model", default="")
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f32s", "f32x", "f16hl", "f16"])
    ap.add_argument("--softmax", action="store_true", help="INFUR_DECODE_SOFTMAX instead of INFUR_DECODE_RAW")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--input", default="-", help="raw bgr24 file (default stdin)")
    ap.add_argument("--labels-out", default="", help="raw class planes, one byte per pixel")
    ap.add_argument("--stats-out", default="-", help="JSON lines (default stdout)")
    a = ap.parse_args(argv)

    from . import _lib
    from .app import RawVideoSource, VideoProcError
    from .processors import Context, FramePath, Model, ModelCmd, class_summary

    ctx = Context(device=a.device, dtype=a.dtype)
    model = Model(ctx)
    if a.synthetic_weights:
        from .weights import synth_blob

        model.control(ModelCmd.LoadBlob(synth_blob()))
    elif a.model:
        model.control(ModelCmd.Load(a.model))
    else:
        ap.error("give --model PATH or --synthetic-weights")

    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    flab = open(a.labels_out, "wb") if a.labels_out else None
    fst = sys.stdout if a.stats_out == "-" else open(a.stats_out, "w")
    src = RawVideoSource(fin, a.width, a.height, close_stream=a.input != "-")
    fp = FramePath(ctx, scale_mode=_lib.SCALE_BILINEAR if a.bilinear else _lib.SCALE_NEAREST)
    decode = _lib.DECODE_SOFTMAX if a.softmax else _lib.DECODE_RAW
    img = src.empty_image()
    n, t0 = 0, time.perf_counter()
    while True:
        try:
            fid = src.read_frame(img)
        except VideoProcError as e:
            if e.kind == "FinishedNormally":
                break
            raise
        s = fp.advance_segments(img, a.scale, decode, want_klass=flab is not None, want_conf=False)
        oh, ow = (s.klass.shape if s.klass is not None else _out_dims(ctx, a.width, a.height, a.scale))
        if flab is not None:
            flab.write(memoryview(s.klass).cast("B"))
        fst.write(json.dumps({"frame": fid, "width": ow, "height": oh, "classes": class_summary(s.stats, ow, oh)}) + "\n")
        n += 1
    for f in (flab, fst):
        if f is not None:
            f.flush()
    el = time.perf_counter() - t0
    sys.stderr.write(f"infur segments: {n} frames in {el:.2f} s ({n / max(el, 1e-9):.1f} frames/s)\n")
    ctx.close()
    return 0


def _out_dims(ctx, w, h, factor):
    import ctypes as C

    ow, oh = C.c_uint32(0), C.c_uint32(0)
    ctx.L.infur_scale_out_dims(w, h, float(factor), C.byref(ow), C.byref(oh))
    return oh.value, ow.value


if __name__ == "__main__":
    raise SystemExit(main())
