#!/usr/bin/env python3
"""What Redact costs, on one MI355X, one context, eager launches.

``infur_redact_dev`` on a 1080 x 1920 frame of random bytes with the smooth class plane (blobs, like a segmentation) -- one class
selected, the same with INVERT, everything selected -- for fill, pixelate 16 and blur r = 2, 16, 64 at passes 1 and 3, out of place,
counts wanted: the time of the whole call between two HIP events (median of 25 after warm-up, with min and max).  Yardstick from the
same sitting: a device-to-device copy of the frame.  The last line is the claim the design makes, blur at r = 64 against r = 2.
    python scripts/redact_rate.py            (prints a markdown table)
    python scripts/redact_rate.py --dry-run  (no device: a small frame, made-up times -- checks the planes and the table code only)"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generator of the test planes)

H, W_ = 1080, 1920
FILL, PIXELATE, BLUR = 0, 1, 2
HEAD = ("| selection | selected pixels | call | us (median of 25) | min .. max |\n"
        "|---|---|---|---|---|")
CALLS = ([("fill", FILL, 0, 0), ("pixelate 16", PIXELATE, 16, 0)] +
         [(f"blur r = {r}, {p} pass{'es' if p > 1 else ''}", BLUR, r, p) for p in (1, 3) for r in (2, 16, 64)])


def selections(plane):
    """(name, table of bytes, INVERT)"""
    one = np.zeros(21, np.uint8)
    one[int(np.bincount(plane.ravel()).argmax())] = 1
    return (("one class", one, 0), ("one class, inverted", one, 1), ("everything", np.zeros(21, np.uint8), 1))


def row(name, n_sel, call, ts):
    return f"| {name} | {n_sel} | {call} | {statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |"


def dry_run(h=54, w=96):
    plane = R.smooth(h, w)
    print(HEAD)
    for name, table, invert in selections(plane):
        for call, _, _, _ in CALLS + [("copy", 0, 0, 0)]:
            print(row(name, int(((table[plane] != 0) != bool(invert)).sum()), call, [3.0, 2.0, 4.0]))


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


def measure(h, w):
    from infur_amd.processors import Context

    plane = R.smooth(h, w)
    frame = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    print(HEAD)
    with Context(device=0) as c:
        L, N, hip, stream = c.L, h * w, hip_runtime(), C.c_void_p(c.stream)
        start, stop = C.c_void_p(None), C.c_void_p(None)
        assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
        b = {}
        for name, n in (("frame", N * 3), ("plane", N), ("select", 21), ("out", N * 3), ("counts", 32)):
            b[name] = C.c_void_p(None)
            c.check(L.infur_dev_alloc(c.h, n, C.byref(b[name])))
        c.check(L.infur_memcpy_h2d(c.h, b["frame"], frame.ctypes.data, frame.nbytes))
        c.check(L.infur_memcpy_h2d(c.h, b["plane"], plane.ctypes.data, plane.nbytes))

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

        medians = {}
        for name, table, invert in selections(plane):
            c.check(L.infur_memcpy_h2d(c.h, b["select"], table.ctypes.data, table.nbytes))
            counts = np.zeros(8, np.uint32)
            for call, mode, size, passes in CALLS:
                ts = timed(lambda: L.infur_redact_dev(c.h, b["frame"], b["plane"], 1, h, w, b["select"], 21, invert, mode, size, passes, 0, b["out"],
                                                      b["counts"]))
                c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, b["counts"], counts.nbytes))
                medians[name, call] = statistics.median(ts)
                print(row(name, int(counts[0]), call, ts), flush=True)
            print(row(name, int(counts[0]), "copy", timed(lambda: hip.hipMemcpyAsync(b["out"], b["frame"], N * 3, 3, stream))), flush=True)  # 3: device to device
        for d in b.values():
            L.infur_dev_free(c.h, d)
    print()
    for name, _, _ in selections(plane):
        for p in ("1 pass", "3 passes"):
            print(f"blur r = 64 / r = 2, {p}, {name}: {medians[name, f'blur r = 64, {p}'] / medians[name, f'blur r = 2, {p}']:.3f}")


def main(argv):
    return dry_run() if "--dry-run" in argv else measure(H, W_)


if __name__ == "__main__":
    main(sys.argv[1:])
