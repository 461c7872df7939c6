#!/usr/bin/env python3
"""What Regions costs, on one MI355X, everything resident in HBM, eager launches.

1. ``infur_regions_dev`` on three 1080p class planes -- smooth (blobs, like a segmentation), one class, uniform noise over three
   classes (the adversarial case for the seam-merge atomics) -- for both connectivities: the time of the whole call (all its
   launches between two HIP events; median of 25 after warm-up) beside a device-to-device copy of the bytes the call has to
   move, h*w*(1 + 1 + 4), and the ratio of the two.
2. Frames/s of the fused ``infur_frame_regions_dev`` beside ``infur_frame_segments_dev`` on the same build in the same run,
   legs alternating, each at least a second and repeated five times, with the segments leg's own run-to-run spread.
    python scripts/regions_rate.py [--quick]        (prints markdown tables)"""
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
LEG_S, REPEATS = (0.3, 3) if QUICK else (1.0, 5)
H, W_ = 1080, 1920
ROWS = 4096


def dev_alloc(c, n):
    d = C.c_void_p(None)
    c.check(c.L.infur_dev_alloc(c.h, n, C.byref(d)))
    return d


def d2d_copy_us(c, nbytes, reps=25):
    """median time of a device-to-device copy of nbytes on the context's stream, HIP events"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    e0, e1 = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    src, dst = dev_alloc(c, nbytes), dev_alloc(c, nbytes)
    stream = C.c_void_p(c.stream)
    ts = []
    for i in range(reps + 5):
        assert hip.hipEventRecord(e0, stream) == 0
        assert hip.hipMemcpyAsync(dst, src, nbytes, 3, stream) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if i >= 5:
            ts.append(ms.value * 1e3)
    for d in (src, dst):
        c.L.infur_dev_free(c.h, d)
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
    return statistics.median(ts)


# ---------------------------------------------------------------- 1. the call on given planes
print("| plane (1080p) | connectivity | regions | infur_regions_dev us (median of 25) | min .. max | D2D copy of h*w*6 bytes, us | ratio |")
print("|---|---|---|---|---|---|---|")
with Context(device=0, profile=True) as c:
    L = c.L
    copy_us = d2d_copy_us(c, H * W_ * 6)
    bufs = {name: dev_alloc(c, n) for name, n in (("klass", H * W_), ("conf", H * W_), ("labels", H * W_ * 4), ("table", ROWS * 80), ("n", 4))}
    for name, plane in (("smooth", R.smooth(H, W_)), ("one class", R.single(H, W_)), ("noise, 3 classes", R.noise(H, W_, 3))):
        conf = R.conf_for(plane)
        c.check(L.infur_memcpy_h2d(c.h, bufs["klass"], plane.ctypes.data, plane.nbytes))
        c.check(L.infur_memcpy_h2d(c.h, bufs["conf"], conf.ctypes.data, conf.nbytes))
        for conn in (4, 8):
            ts = []
            for i in range(30):
                c.check(L.infur_regions_dev(c.h, bufs["klass"], bufs["conf"], H, W_, conn, 0, 0, bufs["labels"], bufs["table"], ROWS, bufs["n"]))
                c.synchronize()
                rec = [r for r in c.profile() if r["kernel"] == "regions"]
                assert rec, "the call left no profile record"  # (records accumulate until the next forward: the last is this call's)
                if i >= 5:
                    ts.append(rec[-1]["ms"] * 1e3)
            n = np.zeros(1, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, bufs["n"], 4))
            us = statistics.median(ts)
            print(f"| {name} | {conn} | {int(n[0])} | {us:.1f} | {min(ts):.1f} .. {max(ts):.1f} | {copy_us:.1f} | {us / copy_us:.1f} x |", flush=True)
    for d in bufs.values():
        L.infur_dev_free(c.h, d)


# ---------------------------------------------------------------- 2. the fused frame path
class Bench:
    def __init__(self, dtype, depth, w, h):
        self.c = Context(device=0, dtype=dtype)
        m = Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.k = m.get_info().num_classes
        self.w, self.h = w, h
        self.bufs = {name: dev_alloc(self.c, n) for name, n in (("bgr", w * h * 3), ("klass", w * h), ("conf", w * h), ("stats", self.k * 64),
                                                                 ("labels", w * h * 4), ("table", ROWS * 80), ("n", 4))}
        fr = W.synth_frame(h, w, index=1)
        self.c.check(self.c.L.infur_memcpy_h2d(self.c.h, self.bufs["bgr"], fr.ctypes.data, fr.nbytes))
        self.ow, self.oh = C.c_uint32(0), C.c_uint32(0)

    def frame(self, leg):
        L, hd, b, w, h = self.c.L, self.c.h, self.bufs, self.w, self.h
        if leg == "segments":
            rc = L.infur_frame_segments_dev(hd, b["bgr"], w, h, 1.0, 0, _lib.DECODE_SOFTMAX, b["klass"], b["conf"], w * h, None, 0, None, 0, None,
                                            C.byref(self.ow), C.byref(self.oh))
        else:
            rc = L.infur_frame_regions_dev(hd, b["bgr"], w, h, 1.0, 0, _lib.DECODE_SOFTMAX, leg, 0, 0, b["klass"], b["conf"], w * h, b["labels"],
                                           w * h * 4, b["table"], ROWS, b["n"], None, C.byref(self.ow), C.byref(self.oh))
        self.c.check(rc)

    def leg_rate(self, leg, n):
        self.c.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.frame(leg)
        self.c.synchronize()
        return n / (time.perf_counter() - t0)

    def close(self):
        for d in self.bufs.values():
            self.c.L.infur_dev_free(self.c.h, d)
        self.c.close()


LEGS = (("advance_segments (SOFTMAX, planes)", "segments"), ("advance_regions, connectivity 8", 8), ("advance_regions, connectivity 4", 4))
print("\n| mode | frame | leg | frames/s (median of %d) | min .. max | vs segments |\n|---|---|---|---|---|---|" % REPEATS)
for dtype, depth, w, h in (("f16hl", 50, W_, H), ("f32", 50, W_, H)):
    b = Bench(dtype, depth, w, h)
    for _, leg in LEGS:  # warm every leg (arena, tile configurations, scratch)
        for _ in range(6):
            b.frame(leg)
    n = max(4, int(b.leg_rate("segments", 8) * LEG_S) + 1)
    rates = {name: [] for name, _ in LEGS}
    for _ in range(REPEATS):
        for name, leg in LEGS:
            rates[name].append(b.leg_rate(leg, n))
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    nreg = np.zeros(1, np.uint32)
    b.c.check(b.c.L.infur_memcpy_d2h(b.c.h, nreg.ctypes.data, b.bufs["n"], 4))
    for name, _ in LEGS:
        r = rates[name]
        print(f"| {dtype} r{depth} | {w}x{h} | {name} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | {100 * (statistics.median(r) / base - 1):+.2f} % |",
              flush=True)
    print(f"| {dtype} r{depth} | {w}x{h} | spread of the segments leg | | {100 * spread:.2f} % of its median | ({int(nreg[0])} regions in the frame) |", flush=True)
    b.close()
