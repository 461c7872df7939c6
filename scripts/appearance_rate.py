#!/usr/bin/env python3
"""What Appearance costs, on one MI355X, one context, eager launches.

``infur_appearance_dev`` on a 1080 x 1920 frame of random bytes, table and histogram wanted, on four planes: the smooth class plane
(blobs, like a segmentation), a one-value plane, a noise byte plane of 48 values (more than a tile keeps in LDS) and a u32 plane with
a value per pixel (every run goes to global memory itself): the time of the whole call between two HIP events (median of 25 after
warm-up, with min and max).  Yardstick from the same sitting: Compare's dense form (runs and LDS counts, 21 x 21) of the smooth
plane against itself.
    python scripts/appearance_rate.py            (prints a markdown table)
    python scripts/appearance_rate.py --dry-run  (no device: a small frame, made-up times -- checks the planes and the table code only)"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generator of the test planes)
from redact_rate import hip_runtime  # noqa: E402

H, W_ = 1080, 1920
HEAD = ("| plane | rows | call | us (median of 25) | min .. max |\n"
        "|---|---|---|---|---|")


def planes(h, w):
    """(name, plane, rows)"""
    return (("smooth", R.smooth(h, w), 21), ("one value", R.single(h, w), 21), ("noise, 48 values", R.noise(h, w, 48), 48),
            ("a value per pixel", np.arange(h * w, dtype=np.uint32).reshape(h, w), h * w))


def row(name, rows, call, ts):
    return f"| {name} | {rows} | {call} | {statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |"


def dry_run(h=54, w=96):
    print(HEAD)
    for name, plane, rows in planes(h, w):
        print(row(name, rows, "appearance", [3.0, 2.0, 4.0]))
    print(row("smooth", 21, "compare (dense)", [3.0, 2.0, 4.0]))


def measure(h, w):
    from infur_amd.processors import Context

    frame = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    print(HEAD)
    with Context(device=0) as c:
        L, N, hip, stream = c.L, h * w, hip_runtime(), C.c_void_p(c.stream)
        start, stop = C.c_void_p(None), C.c_void_p(None)
        assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
        b = {}
        for name, n in (("frame", N * 3), ("plane", N * 4), ("table", N * 96), ("hist", N * 256), ("counts", 32), ("matrix", 21 * 21 * 4)):
            b[name] = C.c_void_p(None)
            c.check(L.infur_dev_alloc(c.h, n, C.byref(b[name])))
        c.check(L.infur_memcpy_h2d(c.h, b["frame"], frame.ctypes.data, frame.nbytes))

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

        for name, plane, rows in reversed(planes(h, w)):  # (the smooth plane last: Compare reads it)
            c.check(L.infur_memcpy_h2d(c.h, b["plane"], plane.ctypes.data, plane.nbytes))
            elem = plane.dtype.itemsize
            print(row(name, rows, "appearance", timed(lambda: L.infur_appearance_dev(c.h, b["frame"], b["plane"], elem, h, w, 0, 0, b["table"], rows,
                                                                                      b["hist"], None))), flush=True)
        print(row("smooth", 21, "compare (dense)", timed(lambda: L.infur_compare_dev(c.h, b["plane"], 1, b["plane"], 1, h, w, 0, 0, 0, b["matrix"], 21, 21,
                                                                                     None, None, b["counts"], 0))), flush=True)
        for d in b.values():
            L.infur_dev_free(c.h, d)


def main(argv):
    return dry_run() if "--dry-run" in argv else measure(H, W_)


if __name__ == "__main__":
    main(sys.argv[1:])
