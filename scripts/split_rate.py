#!/usr/bin/env python3
"""What Split costs, on one MI355X, one context, eager launches.

1. ``infur_split_dev`` (labels, 2^16 table rows and counts wanted, the default slots) on 1080p label planes with the ``dist2``
   ``infur_anchors_dev`` leaves on the device, at core 16 and 144: the time of the whole call (all its launches between two HIP
   events; median of 25 after warm-up) --
     smooth              what a segmentation looks like: a few thousand regions, most of them tiny
     one class           one region whose ridge is a plateau chain as long as a row: the doubling launches all run
     noise, 3 classes    every second pixel a region
   The yardsticks beside it are ``infur_anchors_dev`` and ``infur_sieve_dev`` (min_pixels 64) on the same plane, and a device-to-
   device copy of the plane between two HIP events.
2. PCIe-inclusive frames/s of ``FramePath.advance_split`` beside ``advance_regions`` on the same build in the same run, legs
   alternating, each at least a second and repeated five times, with the regions leg's own run-to-run spread.
    python scripts/split_rate.py [--quick]     (prints markdown tables)
    python scripts/split_rate.py --calls       (the first table alone)
    python scripts/split_rate.py --dry-run     (no device: small planes, the reference's counts, made-up times -- checks the planes
                                                and the table code only; its numbers mean nothing)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generators of the test planes)
import sieve_rate as SR  # noqa: E402  (the device helpers and the frame legs' table)
from infur_amd import _lib  # noqa: E402

H, W_ = 1080, 1920
CORES = (16, 144)
NONE = 0xFFFFFFFF
LEGS = (("advance_regions (planes + labels + table)", "regions"), ("advance_split (class plane, tables, segment plane + counts)", "split"))
CALL_HEAD = ("| plane | regions | core | BASINS | PAIRS | RUNS | MARKED | ROUNDS | SEGMENTS | status | infur_split_dev us (median of 25) | min .. max | "
             "infur_anchors_dev us | infur_sieve_dev us | D2D copy us |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")


def call_row(name, h, w, n, core, c, t, t_anch, t_sieve, t_copy):
    return (f"| {name} {h}x{w} | {n} | {core} | {c[_lib.SPLIT_BASINS]} | {c[_lib.SPLIT_PAIRS]} | {c[_lib.SPLIT_RUNS]} | {c[_lib.SPLIT_MARKED]} | "
            f"{c[_lib.SPLIT_ROUNDS]} | {c[_lib.SPLIT_SEGMENTS]} | {c[_lib.SPLIT_STATUS]} | {statistics.median(t):.1f} | {min(t):.1f} .. {max(t):.1f} | "
            f"{statistics.median(t_anch):.1f} | {statistics.median(t_sieve):.1f} | {statistics.median(t_copy):.1f} |")


def dry_run(h=27, w=48):
    import split_ref as S

    print(CALL_HEAD)
    for name, k in SR.cases(h, w):
        labels, _, n = R.label(k, connectivity=4)
        d2 = S.dist2(labels)
        for core in CORES:
            counts = S.split(labels, d2, core, slots=1024)[2]
            print(call_row(name, h, w, n, core, counts.tolist(), [30.0, 20.0, 40.0], [3.0], [9.0], [2.0]))
    print("\n" + SR.FRAME_HEAD % 3)
    for line in SR.frame_rows("f16hl", 50, w, h, {SR.LEGS[0][0]: [100.0, 101.0, 99.0], SR.LEGS[1][0]: [98.0, 99.0, 97.0]}):
        print(line.replace(SR.LEGS[1][0], LEGS[1][0]))


def timed_copy(c, dst, src, nbytes):
    """-> the microseconds of 25 device-to-device copies after 5 of warm-up, each between two HIP events on the context's stream"""
    import ctypes as C

    hip, stream, ms = C.CDLL("libamdhip64.so"), C.c_void_p(c.stream), C.c_float(0)
    e0, e1 = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    ts = []
    for i in range(30):
        assert hip.hipEventRecord(e0, stream) == 0
        assert hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, stream) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if i >= 5:
            ts.append(ms.value * 1e3)
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
    return ts


def measure_calls(h, w):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    rows = 1 << 16
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, k in SR.cases(h, w):
            b = {key: SR.dev_alloc(c, n) for key, n in (("klass", h * w), ("labels", h * w * 4), ("n", 4), ("d2", h * w * 4), ("seg", h * w * 4),
                                                         ("table", rows * 24), ("counts", 32), ("out", h * w), ("sc", 32))}
            c.check(L.infur_memcpy_h2d(c.h, b["klass"], k.ctypes.data, k.nbytes))
            c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, 4, 0, 0, b["labels"], None, 0, b["n"]))
            n = np.zeros(1, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, b["n"], 4))
            n = int(n[0])
            b["rtable"] = SR.dev_alloc(c, n * 80)
            c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, 4, 0, 0, b["labels"], b["rtable"], n, b["n"]))
            t_anch = SR.timed(c, "anchors", lambda: L.infur_anchors_dev(c.h, b["labels"], 4, h, w, 1, NONE, b["d2"], None, 0))
            t_sieve = SR.timed(c, "sieve", lambda: L.infur_sieve_dev(c.h, b["klass"], b["labels"], b["rtable"], n, b["n"], h, w, 64, 0, 0, b["out"], None, b["sc"]))
            t_copy = timed_copy(c, b["seg"], b["labels"], h * w * 4)
            for core in CORES:
                t = SR.timed(c, "split", lambda: L.infur_split_dev(c.h, b["labels"], 4, b["d2"], h, w, 1, NONE, core, 0, b["seg"], b["table"], rows, b["counts"]))
                counts = np.empty(8, np.uint32)
                c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, b["counts"], 32))
                print(call_row(name, h, w, n, core, counts.tolist(), t, t_anch, t_sieve, t_copy), flush=True)
            for d in b.values():
                L.infur_dev_free(c.h, d)


class Bench(SR.Bench):
    def frame(self, leg):
        if leg == "regions":
            self.fp.advance_regions(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        else:
            self.fp.advance_split(self.frame_in, CORES[0], 1.0, _lib.DECODE_SOFTMAX, want_labels=True, want_conf=True)


def measure_frames(leg_s, repeats):
    print("\n" + SR.FRAME_HEAD % repeats)
    for dtype, depth, w, h in (("f16hl", 50, W_, H),):
        b = Bench(dtype, depth, w, h)
        for _, leg in LEGS:
            for _ in range(6):
                b.frame(leg)
        n = max(4, int(b.leg_rate("regions", 8) * leg_s) + 1)
        rates = {name: [] for name, _ in SR.LEGS}
        for _ in range(repeats):
            for (name, _), (_, leg) in zip(SR.LEGS, LEGS):
                rates[name].append(b.leg_rate(leg, n))
        for line in SR.frame_rows(dtype, depth, w, h, rates):
            print(line.replace(SR.LEGS[1][0], LEGS[1][0]), flush=True)
        b.close()


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    quick = (0.3, 3) if "--quick" in argv else (1.0, 5)
    measure_calls(H, W_)
    if "--calls" not in argv:
        measure_frames(*quick)


if __name__ == "__main__":
    main(sys.argv[1:])
