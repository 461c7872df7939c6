#!/usr/bin/env python3
"""What Anchors costs, on one MI355X, one context, eager launches.

1. ``infur_anchors_dev`` on 1080p planes -- smooth (blobs, like a segmentation), one class (the worst case of the column walk:
   its length is the pixel's own distance, up to 540 here), uniform noise over three classes -- as class bytes, both outputs
   wanted: the time of the whole call (its memset and three launches between two HIP events; median of 25 after warm-up) with
   the largest dist2 of the plane and the mean length of the walk.
2. PCIe-inclusive frames/s of ``FramePath.advance_anchors`` -- with the 8 MB plane of distances coming back, and with the anchor
   rows alone -- beside ``advance_regions`` on the same build in the same run, legs alternating, each at least a second and
   repeated five times, with the regions leg's own run-to-run spread.
3. ``--legs``: frames/s of the legs that existed before Anchors (``advance_segments``, ``advance_regions``, ``advance_tracks``),
   one line per leg and mode, for comparing two builds in one sitting (--root selects the checkout whose package and library run).
    python scripts/anchors_rate.py [--quick]     (prints markdown tables)
    python scripts/anchors_rate.py --legs [--quick] [--root CHECKOUT]
    python scripts/anchors_rate.py --dry-run     (no device: small planes, the reference's distances, made-up times -- checks
                                                  the planes and the table code only; its numbers mean nothing)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # --legs on another checkout of the project (its package and its library), e.g. the parent commit's
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generators of the test planes)
from infur_amd import _lib  # noqa: E402

H, W_ = 1080, 1920
LEGS = (("advance_regions (planes + table)", "regions"), ("advance_anchors (the same + dist2 + anchors)", "anchors"),
        ("advance_anchors, want_dist2=False (the same + anchors)", "anchors_only"))
OLD_LEGS = ("segments", "regions", "tracks")
CALL_HEAD = ("| plane | largest dist2 | mean walk, steps | infur_anchors_dev us (median of 25) | min .. max |\n"
             "|---|---|---|---|---|")
FRAME_HEAD = "| mode | frame | leg | frames/s (median of %d) | min .. max | vs regions |\n|---|---|---|---|---|---|"


# ---------------------------------------------------------------- planes and tables: no device needed
def planes(h, w):
    return (("smooth", R.smooth(h, w)), ("one class", R.single(h, w)), ("noise, 3 classes", R.noise(h, w, 3)))


def call_row(name, h, w, dmax, walk, ts):
    return f"| {name} {h}x{w} | {dmax} | {walk:.1f} | {statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |"


def frame_rows(dtype, depth, w, h, rates):
    """rates: {leg name: [frames/s per repeat]} -> the table rows of one mode and frame size"""
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    out = []
    for name, _ in LEGS:
        r = rates[name]
        out.append(f"| {dtype} r{depth} | {w}x{h} | {name} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | "
                   f"{100 * (statistics.median(r) / base - 1):+.2f} % |")
    out.append(f"| spread of the regions leg, {dtype} | {w}x{h} | | | {100 * spread:.2f} % of its median | |")
    return out


def mean_walk(dist2):
    """the steps of the column walk per pixel: up and down it stops at the first dy with dy^2 >= dist2"""
    return float(np.ceil(np.sqrt(dist2.astype(np.float64))).mean())


def dry_run(h=54, w=96):
    import anchors_ref as A

    print(CALL_HEAD)
    for name, plane in planes(h, w):
        d = A.distance(plane)
        print(call_row(name, h, w, int(d.max()), mean_walk(d), [3.0, 2.0, 4.0]))
    print("\n" + FRAME_HEAD % 3)
    for dtype in ("f16hl", "f32"):
        for line in frame_rows(dtype, 50, w, h, {LEGS[0][0]: [100.0, 101.0, 99.0], LEGS[1][0]: [98.0, 99.0, 97.0], LEGS[2][0]: [99.0, 99.5, 98.5]}):
            print(line)


# ---------------------------------------------------------------- the device
def dev_alloc(c, n):
    d = C.c_void_p(None)
    c.check(c.L.infur_dev_alloc(c.h, n, C.byref(d)))
    return d


def measure_calls(h, w, rows=256):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    with Context(device=0, profile=True) as c:
        L, N = c.L, h * w
        bufs = {name: dev_alloc(c, n) for name, n in (("plane", N), ("dist2", N * 4), ("anchors", rows * 8))}
        for name, plane in planes(h, w):
            c.check(L.infur_memcpy_h2d(c.h, bufs["plane"], plane.ctypes.data, plane.nbytes))
            ts = []
            for i in range(30):
                c.check(L.infur_anchors_dev(c.h, bufs["plane"], 1, h, w, 0, 0, bufs["dist2"], bufs["anchors"], rows))
                c.synchronize()
                rec = [r for r in c.profile() if r["kernel"] == "anchors"]
                assert rec, "the call left no profile record"  # (records accumulate until the next forward: the last is this call's)
                if i >= 5:
                    ts.append(rec[-1]["ms"] * 1e3)
            d = np.empty((h, w), np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, d.ctypes.data, bufs["dist2"], d.nbytes))
            print(call_row(name, h, w, int(d.max()), mean_walk(d), ts), flush=True)
        for d in bufs.values():
            L.infur_dev_free(c.h, d)


class Bench:
    """the host-pointer frame paths on one context: everything they return crosses PCIe"""

    def __init__(self, dtype, depth, w, h):
        from infur_amd import weights as W
        from infur_amd.processors import Context, FramePath, Model, ModelCmd, Tracks

        self.c = Context(device=0, dtype=dtype)
        Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.fp = FramePath(self.c)
        self.tracks = Tracks(self.c)
        self.frame_in = W.synth_frame(h, w, index=1)

    def frame(self, leg):
        if leg == "segments":
            self.fp.advance_segments(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        elif leg == "regions":
            self.fp.advance_regions(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        elif leg == "tracks":
            self.fp.advance_tracks(self.tracks, self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        else:
            self.fp.advance_anchors(self.frame_in, 1.0, _lib.DECODE_SOFTMAX, want_dist2=leg != "anchors_only")

    def leg_rate(self, leg, n):
        self.c.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.frame(leg)  # (the host-pointer calls synchronise themselves)
        return n / (time.perf_counter() - t0)

    def close(self):
        self.c.close()


def measure_frames(leg_s, repeats):
    print("\n" + FRAME_HEAD % repeats)
    for dtype, depth, w, h in (("f16hl", 50, W_, H), ("f32", 50, W_, H)):
        b = Bench(dtype, depth, w, h)
        for _, leg in LEGS:  # warm every leg (arena, tile configurations, scratch)
            for _ in range(6):
                b.frame(leg)
        n = max(4, int(b.leg_rate("regions", 8) * leg_s) + 1)
        rates = {name: [] for name, _ in LEGS}
        for _ in range(repeats):
            for name, leg in LEGS:
                rates[name].append(b.leg_rate(leg, n))
        for line in frame_rows(dtype, depth, w, h, rates):
            print(line, flush=True)
        b.close()


def measure_old_legs(leg_s, repeats):
    """one line per leg and mode: `legs <library> <mode> <leg> median min max`"""
    for dtype in ("f16hl", "f32"):
        b = Bench(dtype, 50, W_, H)
        for leg in OLD_LEGS:
            for _ in range(6):
                b.frame(leg)
        n = max(4, int(b.leg_rate("segments", 8) * leg_s) + 1)
        rates = {leg: [] for leg in OLD_LEGS}
        for _ in range(repeats):
            for leg in OLD_LEGS:
                rates[leg].append(b.leg_rate(leg, n))
        for leg in OLD_LEGS:
            r = rates[leg]
            print(f"legs {ROOT} {dtype} {leg} {statistics.median(r):.2f} {min(r):.2f} {max(r):.2f}", flush=True)
        b.close()


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    quick = (0.3, 3) if "--quick" in argv else (1.0, 5)
    if "--legs" in argv:
        return measure_old_legs(*quick)
    measure_calls(H, W_)
    measure_frames(*quick)


if __name__ == "__main__":
    main(sys.argv[1:])
