#!/usr/bin/env python3
"""Frame rate of the Segments frame path (infur_frame_segments_dev) against the existing shade path (infur_frame_advance_dev), in
one process, frames and outputs resident in HBM, eager launches.  Legs alternate shade / RAW planes / SOFTMAX everything /
SOFTMAX planes + statistics; every shape is warmed first, a leg runs for at least a second and is repeated five times; the
run-to-run spread of the shade path is printed beside the medians.  A second, profiled pass prints the per-launch time
(HIP events) of upsample_argmax_segments beside upsample_argmax_shade and the new kernel's achieved GB/s.
    python scripts/segments_rate.py [--quick]        (on an MI355X; prints markdown tables)"""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infur_amd import _lib, weights as W  # noqa: E402
from infur_amd.processors import Context, Model, ModelCmd  # noqa: E402

QUICK = "--quick" in sys.argv
LEG_S, REPEATS = (0.3, 3) if QUICK else (1.0, 5)
CONFIGS = (("f32", 50, 1920, 1080), ("f16hl", 50, 1920, 1080), ("f16", 101, 3840, 2160))
LEGS = (("shade (existing)", None), ("RAW, planes", (_lib.DECODE_RAW, 1, 1, 0, 0)), ("SOFTMAX, all outputs", (_lib.DECODE_SOFTMAX, 1, 1, 1, 1)),
        ("SOFTMAX, planes + stats", (_lib.DECODE_SOFTMAX, 1, 1, 1, 0)))


class Bench:
    def __init__(self, dtype, depth, w, h, profile=False):
        self.c = Context(device=0, dtype=dtype, profile=profile)
        m = Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.k = m.get_info().num_classes
        self.w, self.h = w, h
        L, hd = self.c.L, self.c.h
        self.bufs = {}
        for name, n in (("bgr", w * h * 3), ("rgba", w * h * 4), ("klass", w * h), ("conf", w * h), ("stats", self.k * 64)):
            d = C.c_void_p(None)
            self.c.check(L.infur_dev_alloc(hd, n, C.byref(d)))
            self.bufs[name] = d
        fr = W.synth_frame(h, w, index=1)
        self.c.check(L.infur_memcpy_h2d(hd, self.bufs["bgr"], fr.ctypes.data, fr.nbytes))
        self.ow, self.oh = C.c_uint32(0), C.c_uint32(0)

    def frame(self, leg):
        L, hd, b, w, h = self.c.L, self.c.h, self.bufs, self.w, self.h
        if leg is None:
            rc = L.infur_frame_advance_dev(hd, b["bgr"], w, h, 1.0, 0, b["rgba"], w * h * 4, None, C.byref(self.ow), C.byref(self.oh))
        else:
            decode, kl, cf, st, rg = leg
            rc = L.infur_frame_segments_dev(hd, b["bgr"], w, h, 1.0, 0, decode, b["klass"] if kl else None, b["conf"] if cf else None, w * h,
                                            b["stats"] if st else None, self.k, b["rgba"] if rg else None, w * h * 4, None,
                                            C.byref(self.ow), C.byref(self.oh))
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


print("| mode | frame | leg | frames/s (median of %d) | min .. max | vs shade |\n|---|---|---|---|---|---|" % REPEATS)
for dtype, depth, w, h in CONFIGS:
    b = Bench(dtype, depth, w, h)
    for _, leg in LEGS:  # warm every shape and every leg (arena, tile configurations)
        for _ in range(6):
            b.frame(leg)
    n = max(4, int(b.leg_rate(None, 8) * LEG_S) + 1)  # frames for about LEG_S seconds
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
    print(f"| {dtype} r{depth} | {w}x{h} | spread of the shade path | | {100 * spread:.2f} % of its median | allowed loss: {max(2.0, 100 * spread):.2f} % |", flush=True)
    b.close()

print("\n| mode | frame | kernel | outputs | us per launch (median of 9, HIP events) | GB/s |\n|---|---|---|---|---|---|")
for dtype, depth, w, h in CONFIGS[:2] if QUICK else CONFIGS:
    b = Bench(dtype, depth, w, h, profile=True)
    for name, leg in LEGS:
        ts, by = [], 0.0
        for i in range(12):
            b.frame(leg)
            b.c.synchronize()
            rec = [r for r in b.c.profile() if r["kernel"] in ("upsample_argmax_shade", "upsample_argmax_segments")]
            assert len(rec) == 1, rec
            if i >= 3:
                ts.append(rec[0]["ms"] * 1e3)
                by = rec[0]["bytes"]
        us = statistics.median(ts)
        print(f"| {dtype} r{depth} | {w}x{h} | {rec[0]['kernel']} | {name} | {us:.1f} | {by / us / 1e3:.0f} |", flush=True)
    b.close()
