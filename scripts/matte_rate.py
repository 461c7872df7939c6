#!/usr/bin/env python3
"""What Matte and Composite cost, on one MI355X, one context, eager launches.

``infur_matte_dev`` on a 1080 x 1920 frame of random bytes, alpha and counts wanted, sigma 24, radius 4, 8 and 16: with the smooth
class plane (blobs, like a segmentation; one class selected), with a noise plane on which no window is uniform (the worst case: every
wave runs the tap loop), and with a one-value plane (the quiet shortcut alone).  ``infur_composite_dev`` in its three modes beside a
device-to-device copy of the frame from the same sitting.  Each time is the whole call between two HIP events (median of 25 after 5
warm calls, with min and max).  The noise rows also say taps per second: the clipped windows' pixels over the time.
    python scripts/matte_rate.py            (prints a markdown table)
    python scripts/matte_rate.py --dry-run  (no device: a small frame, made-up times -- checks the planes and the table code only)"""
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
RADII, SIGMA = (4, 8, 16), 24
HEAD = ("| call | plane | selected pixels | soft pixels | us (median of 25) | min .. max | taps/s |\n"
        "|---|---|---|---|---|---|---|")
MODES = (("colour", 0), ("image", 1), ("cutout", 2))


def planes(h, w):
    """(name, plane, table of bytes)"""
    smooth = R.smooth(h, w)
    one = np.zeros(21, np.uint8)
    one[int(np.bincount(smooth.ravel()).argmax())] = 1
    return (("smooth", smooth, one), ("noise", R.noise(h, w, 2, seed=1), np.array([0, 1], np.uint8)), ("one value", np.zeros((h, w), np.uint8), np.ones(1, np.uint8)))


def taps(h, w, r):
    """the pixels of all windows, clipped at the frame"""
    side = lambda n: sum(min(n - 1, i + r) - max(0, i - r) + 1 for i in range(n))  # noqa: E731
    return side(h) * side(w)


def row(call, plane, counts, ts, n_taps=0):
    med = statistics.median(ts)
    return f"| {call} | {plane} | {counts[0]} | {counts[3]} | {med:.1f} | {min(ts):.1f} .. {max(ts):.1f} | {n_taps / med * 1e6:.3g} |" if n_taps else \
        f"| {call} | {plane} | {counts[0]} | {counts[3]} | {med:.1f} | {min(ts):.1f} .. {max(ts):.1f} | |"


def dry_run(h=54, w=96):
    print(HEAD)
    for name, plane, table in planes(h, w):
        for r in RADII:
            print(row(f"matte r = {r}", name, [int((table[plane] != 0).sum()), 0, 0, 0], [3.0, 2.0, 4.0], taps(h, w, r) if name == "noise" else 0))
    for name, _ in MODES + (("copy", 0),):
        print(row(f"composite {name}" if name != "copy" else name, "", ["", "", "", ""], [3.0, 2.0, 4.0]))


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

    frame = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
    print(HEAD)
    with Context(device=0) as c:
        L, N, hip, stream = c.L, h * w, hip_runtime(), C.c_void_p(c.stream)
        start, stop = C.c_void_p(None), C.c_void_p(None)
        assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
        b = {}
        for name, n in (("frame", N * 3), ("plane", N), ("select", 21), ("alpha", N), ("back", N * 3), ("out", N * 4), ("counts", 32)):
            b[name] = C.c_void_p(None)
            c.check(L.infur_dev_alloc(c.h, n, C.byref(b[name])))
        c.check(L.infur_memcpy_h2d(c.h, b["frame"], frame.ctypes.data, frame.nbytes))
        back = np.ascontiguousarray(frame[::-1])  # (kept in a name: the copy below reads it)
        c.check(L.infur_memcpy_h2d(c.h, b["back"], back.ctypes.data, back.nbytes))

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

        counts = np.zeros(8, np.uint32)
        for name, plane, table in planes(h, w):
            c.check(L.infur_memcpy_h2d(c.h, b["plane"], plane.ctypes.data, plane.nbytes))
            c.check(L.infur_memcpy_h2d(c.h, b["select"], table.ctypes.data, table.nbytes))
            for r in RADII:
                ts = timed(lambda: L.infur_matte_dev(c.h, b["frame"], b["plane"], 1, h, w, b["select"], table.size, 0, None, r, SIGMA, b["alpha"], b["counts"]))
                c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, b["counts"], counts.nbytes))
                print(row(f"matte r = {r}", name, counts, ts, taps(h, w, r) if name == "noise" else 0), flush=True)
        for name, mode in MODES:  # (alpha: the one-value plane's, radius 16; the cost of a pointwise pass does not depend on it)
            print(row(f"composite {name}", "", ["", "", "", ""], timed(lambda: L.infur_composite_dev(c.h, b["frame"], b["alpha"], h, w, mode, b["back"], 0x336699, b["out"]))),
                  flush=True)
        print(row("copy", "", ["", "", "", ""], timed(lambda: hip.hipMemcpyAsync(b["out"], b["frame"], N * 3, 3, stream))), flush=True)  # 3: device to device
        for d in b.values():
            L.infur_dev_free(c.h, d)


def main(argv):
    return dry_run() if "--dry-run" in argv else measure(H, W_)


if __name__ == "__main__":
    main(sys.argv[1:])
