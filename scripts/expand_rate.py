#!/usr/bin/env python3
"""What Expand costs, on one MI355X, one context, eager launches.

``infur_expand_dev`` on 1080p byte planes -- smooth (blobs, like a segmentation) with its background class open, one seed pixel in
a corner (every distance long: what a column walk whose cost is the pixel's own distance is worst at), uniform noise over three
classes with one class open -- at reach 0 and reach 16, every output wanted: the time of the whole call between two HIP events
(median of 25 after warm-up, with min and max).  Yardsticks from the same sitting: ``infur_anchors_dev`` on the same planes and a
device-to-device copy of the plane.
    python scripts/expand_rate.py            (prints a markdown table)
    python scripts/expand_rate.py --dry-run  (no device: small planes, made-up times -- checks the planes and the table code only)"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generators of the test planes)

H, W_ = 1080, 1920
HEAD = ("| plane | open pixels | largest dist2 | call | us (median of 25) | min .. max |\n"
        "|---|---|---|---|---|---|")


def planes(h, w):
    """(name, byte plane, open value)"""
    smooth, corner = R.smooth(h, w), np.zeros((h, w), np.uint8)
    corner[0, 0] = 3
    return (("smooth, background open", smooth, int(np.bincount(smooth.ravel()).argmax())), ("one seed in a corner", corner, 0),
            ("noise, 3 classes, one open", R.noise(h, w, 3), 0))


def row(name, n_open, dmax, call, ts):
    return f"| {name} | {n_open} | {dmax} | {call} | {statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |"


def dry_run(h=54, w=96):
    print(HEAD)
    for name, plane, open_value in planes(h, w):
        for call in ("expand, reach 0", "expand, reach 16", "anchors", "copy"):
            print(row(name, int((plane == open_value).sum()), 0, call, [3.0, 2.0, 4.0]))


def hip_runtime():
    """the HIP runtime this process already runs on (the one mapped file, not a second copy)"""
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def measure(h, w, rows=256):
    from infur_amd.processors import Context

    print(HEAD)
    with Context(device=0) as c:
        L, N, hip, stream = c.L, h * w, hip_runtime(), C.c_void_p(c.stream)
        start, stop = C.c_void_p(None), C.c_void_p(None)
        assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
        b = {}
        for name, n in (("plane", N), ("out", N), ("dist2", N * 4), ("source", N * 4), ("table", rows * 16), ("counts", 32), ("anchors", rows * 8)):
            b[name] = C.c_void_p(None)
            c.check(L.infur_dev_alloc(c.h, n, C.byref(b[name])))

        def timed(call):
            ts = []
            for i in range(30):
                assert hip.hipEventRecord(start, stream) == 0
                assert call() == 0
                assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
                ms = C.c_float(0)
                assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
                if i >= 5:
                    ts.append(ms.value * 1e3)
            return ts

        for name, plane, open_value in planes(h, w):
            c.check(L.infur_memcpy_h2d(c.h, b["plane"], plane.ctypes.data, plane.nbytes))
            n_open, d = int((plane == open_value).sum()), np.empty((h, w), np.uint32)
            for reach in (0, 16):
                ts = timed(lambda: L.infur_expand_dev(c.h, b["plane"], 1, h, w, 0, open_value, reach, b["out"], b["dist2"], b["source"], b["table"], rows,
                                                      b["counts"]))
                c.check(L.infur_memcpy_d2h(c.h, d.ctypes.data, b["dist2"], d.nbytes))
                print(row(name, n_open, int(d.max()), f"expand, reach {reach}", ts), flush=True)
            ts = timed(lambda: L.infur_anchors_dev(c.h, b["plane"], 1, h, w, 0, 0, b["dist2"], b["anchors"], rows))
            c.check(L.infur_memcpy_d2h(c.h, d.ctypes.data, b["dist2"], d.nbytes))
            print(row(name, n_open, int(d.max()), "anchors", ts), flush=True)
            print(row(name, n_open, 0, "copy", timed(lambda: hip.hipMemcpyAsync(b["out"], b["plane"], N, 3, stream))), flush=True)  # 3: device to device
        for d in b.values():
            L.infur_dev_free(c.h, d)


def main(argv):
    return dry_run() if "--dry-run" in argv else measure(H, W_)


if __name__ == "__main__":
    main(sys.argv[1:])
