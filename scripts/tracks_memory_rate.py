#!/usr/bin/env python3
"""What Tracks' memory costs, on one MI355X, everything resident in HBM, eager launches.  The method is scripts/tracks_rate.py's.

1. ``infur_tracks_dev`` on two pairs of 1080p planes labelled on the device by ``infur_regions_dev`` -- smooth blobs shifted by
   (1, 2) pixels per frame, and a flicker pair (the smooth plane, and the same with class 1 painted as class 2, so that every
   step loses and revives some hundred tracks) -- the step alternating between the two frames of a pair.  HIP events around the
   whole step, median of 25 after warm-up, with memory off and with memory on (``max_lost`` 2, ``reach`` 8).
2. Frames/s of the fused ``infur_frame_tracks_dev`` for f16hl with memory off and on beside ``infur_frame_regions_dev``, legs
   alternating, each at least a second and repeated five times, with the regions leg's own run-to-run spread.

``--off-only`` leaves out everything that needs the memory calls: run on a checkout of the parent commit (twice) it gives the
numbers the memory-off rows must match within the larger of 2 % and the difference of those two runs.
    python scripts/tracks_memory_rate.py [--quick] [--off-only]        (prints markdown tables)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generators of the test planes)
from infur_amd import _lib, weights as W  # noqa: E402
from infur_amd.processors import Context, Model, ModelCmd  # noqa: E402

QUICK = "--quick" in sys.argv
OFF_ONLY = "--off-only" in sys.argv
LEG_S, REPEATS = (0.3, 3) if QUICK else (1.0, 5)
H, W_ = 1080, 1920
ROWS = 65536
MAX_LOST, REACH = 2, 8
MODES = (("off", False),) if OFF_ONLY else (("off", False), (f"on (max_lost {MAX_LOST}, reach {REACH})", True))


def dev_alloc(c, n):
    d = C.c_void_p(None)
    c.check(c.L.infur_dev_alloc(c.h, n, C.byref(d)))
    return d


def tracker(c, memory):
    trk = C.c_void_p(None)
    c.check(c.L.infur_tracker_create(c.h, 0, 0, C.byref(trk)))
    if memory:
        c.check(c.L.infur_tracker_set_memory(trk, MAX_LOST, REACH, 0))
    return trk


# ---------------------------------------------------------------- 1. the step on given planes
print("| planes (1080p) | memory | regions | summary of the last step | memory summary (revived, lost, expired, held) "
      "| infur_tracks_dev us (median of 25) | min .. max |")
print("|---|---|---|---|---|---|---|")
with Context(device=0, profile=True) as c:
    L = c.L
    klass = dev_alloc(c, H * W_)
    frames = [{name: dev_alloc(c, n) for name, n in (("labels", H * W_ * 4), ("table", ROWS * 80), ("n", 4))} for _ in range(2)]
    outs = {name: dev_alloc(c, n) for name, n in (("tor", ROWS * 4), ("plane", H * W_ * 4), ("ttab", ROWS * 64), ("summary", 16))}
    smooth = R.smooth(H, W_)
    painted = smooth.copy()
    painted[smooth == 1] = 2
    for name, pair in (("smooth, shifted by (1, 2)", (smooth, np.roll(smooth, (1, 2), axis=(0, 1)))), ("smooth, class 1 flickers", (smooth, painted))):
        for f, plane in zip(frames, pair):
            plane = np.ascontiguousarray(plane)
            c.check(L.infur_memcpy_h2d(c.h, klass, plane.ctypes.data, plane.nbytes))
            c.check(L.infur_regions_dev(c.h, klass, None, H, W_, 8, 0, 0, f["labels"], f["table"], ROWS, f["n"]))
            c.synchronize()
        for mode, memory in MODES:
            trk = tracker(c, memory)
            ts = []
            for i in range(30):
                f = frames[i & 1]
                c.check(L.infur_tracks_dev(trk, f["labels"], f["table"], ROWS, f["n"], H, W_, 1, outs["tor"], outs["plane"], outs["ttab"], outs["summary"]))
                c.synchronize()
                rec = [r for r in c.profile() if r["kernel"] == "tracks"]
                assert rec, "the step left no profile record"  # (records accumulate until the next forward: the last is this step's)
                if i >= 5:
                    ts.append(rec[-1]["ms"] * 1e3)
            n, summary, msum = np.zeros(1, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, frames[1]["n"], 4))
            c.check(L.infur_memcpy_d2h(c.h, summary.ctypes.data, outs["summary"], 16))
            if memory:
                c.check(L.infur_tracker_memory(trk, None, 0, msum.ctypes.data, None, 0))
            L.infur_tracker_destroy(trk)
            print(f"| {name} | {mode} | {int(n[0])} | {summary.tolist()} | {msum.tolist() if memory else '-'} | {statistics.median(ts):.1f} "
                  f"| {min(ts):.1f} .. {max(ts):.1f} |", flush=True)
    for d in [klass] + [p for f in frames for p in f.values()] + list(outs.values()):
        L.infur_dev_free(c.h, d)


# ---------------------------------------------------------------- 2. the fused frame path
class Bench:
    def __init__(self, dtype, depth, w, h):
        self.c = Context(device=0, dtype=dtype)
        Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.w, self.h = w, h
        self.bufs = {name: dev_alloc(self.c, n) for name, n in (("bgr", w * h * 3), ("klass", w * h), ("conf", w * h), ("labels", w * h * 4),
                                                                 ("table", ROWS * 80), ("n", 4), ("tor", ROWS * 4), ("plane", w * h * 4),
                                                                 ("ttab", ROWS * 64), ("summary", 16))}
        fr = W.synth_frame(h, w, index=1)
        self.c.check(self.c.L.infur_memcpy_h2d(self.c.h, self.bufs["bgr"], fr.ctypes.data, fr.nbytes))
        self.ow, self.oh = C.c_uint32(0), C.c_uint32(0)
        self.trk = {"tracks": tracker(self.c, False)}
        if not OFF_ONLY:
            self.trk["tracks+memory"] = tracker(self.c, True)

    def frame(self, leg):
        L, hd, b, w, h = self.c.L, self.c.h, self.bufs, self.w, self.h
        args = (hd, b["bgr"], w, h, 1.0, 0, _lib.DECODE_SOFTMAX, 8, 0, 0, b["klass"], b["conf"], w * h, b["labels"], w * h * 4, b["table"], ROWS, b["n"],
                None, C.byref(self.ow), C.byref(self.oh))
        if leg == "regions":
            rc = L.infur_frame_regions_dev(*args)
        else:
            rc = L.infur_frame_tracks_dev(*args, self.trk[leg], 1, b["tor"], None, b["ttab"], b["summary"])
        self.c.check(rc)

    def leg_rate(self, leg, n):
        self.c.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.frame(leg)
        self.c.synchronize()
        return n / (time.perf_counter() - t0)

    def close(self):
        for t in self.trk.values():
            self.c.L.infur_tracker_destroy(t)
        for d in self.bufs.values():
            self.c.L.infur_dev_free(self.c.h, d)
        self.c.close()


LEGS = (("frame_regions_dev, connectivity 8", "regions"), ("frame_tracks_dev (ids, table, summary), memory off", "tracks")) + \
    (() if OFF_ONLY else ((f"frame_tracks_dev, memory on (max_lost {MAX_LOST}, reach {REACH})", "tracks+memory"),))
print("\n| mode | frame | leg | frames/s (median of %d) | min .. max | vs regions |\n|---|---|---|---|---|---|" % REPEATS)
for dtype, depth, w, h in (("f16hl", 50, W_, H),):
    b = Bench(dtype, depth, w, h)
    for _, leg in LEGS:  # warm every leg (arena, tile configurations, scratch)
        for _ in range(6):
            b.frame(leg)
    n = max(4, int(b.leg_rate("regions", 8) * LEG_S) + 1)
    rates = {name: [] for name, _ in LEGS}
    for _ in range(REPEATS):
        for name, leg in LEGS:
            rates[name].append(b.leg_rate(leg, n))
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    for name, _ in LEGS:
        r = rates[name]
        print(f"| {dtype} r{depth} | {w}x{h} | {name} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | {100 * (statistics.median(r) / base - 1):+.2f} % |",
              flush=True)
    print(f"| {dtype} r{depth} | {w}x{h} | spread of the regions leg | | {100 * spread:.2f} % of its median | |", flush=True)
    b.close()
