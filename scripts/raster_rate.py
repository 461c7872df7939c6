#!/usr/bin/env python3
"""What Raster costs, on one MI355X, one context, eager launches.

1. ``infur_raster_dev`` on 1080p class planes, a byte plane and the counts wanted: the time of the whole call (its memset and
   launches between two HIP events, from the profile record the call leaves; median of 25 after warm-up) on
     smooth, as is       the loops ``infur_outlines_dev`` leaves for what a segmentation looks like: pixel staircases, |dy| = 1
     smooth, 1 px        the same loops behind ``infur_simplify_dev`` at tol16 = 16: chords a few rows long
     checkerboard        every pixel a loop of four vertices and every pixel side a crossing: the worst case
   and ``infur_raster_runs_dev`` on the records ``infur_runs_dev`` leaves for the same planes.
2. Two figures to read them against: the same call with no loop at all -- the memset, the row pass and the finish launch alone,
   24 to 28 bytes per pixel of traffic, the floor of every call -- and ``infur_memcpy_h2d`` of the dense plane from pageable host
   memory, the copy that Raster replaces.
3. ``polygon_fidelity`` of ``smooth(270, 480)`` at 0.5, 1 and 2 px, loop by loop (Simplify) and shared (Coverage).
    python scripts/raster_rate.py              (prints markdown tables)
    python scripts/raster_rate.py --fidelity   (the last table alone)"""
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
from infur_amd import _lib  # noqa: E402

H, W_ = 1080, 1920
HEAD = "| input | records | vertices | painted | conflict | us (median of 25) | min .. max |\n|---|---|---|---|---|---|---|"


def dev_alloc(c, n):
    d = C.c_void_p(None)
    c.check(c.L.infur_dev_alloc(c.h, max(n, 4), C.byref(d)))
    return d


def timed(c, name, call):
    """-> the microseconds of 25 calls after 5 of warm-up, from the profile records the call leaves"""
    ts = []
    for i in range(30):
        c.check(call())
        c.synchronize()
        rec = [r for r in c.profile() if r["name"] == name]
        assert rec, "the call left no profile record"  # (records accumulate until the next forward: the last is this call's)
        if i >= 5:
            ts.append(rec[-1]["ms"] * 1e3)
    return ts


def words(c, d, n):
    out = np.zeros(n, np.uint32)
    c.check(c.L.infur_memcpy_d2h(c.h, out.ctypes.data, d, out.nbytes))
    return out


def row(name, records, vertices, counts, ts):
    return (f"| {name} | {records} | {vertices} | {counts[_lib.RASTER_PAINTED]} | {counts[_lib.RASTER_CONFLICT]} | {statistics.median(ts):.1f} | "
            f"{min(ts):.1f} .. {max(ts):.1f} |")


def measure(h, w):
    from infur_amd.processors import Context

    print(HEAD)
    npix = h * w
    with Context(device=0, profile=True) as c:
        L = c.L
        b = {key: dev_alloc(c, n) for key, n in (("plane", npix), ("out", npix), ("oc", 12), ("sc", 16), ("rc", 16), ("n", 4), ("zero", 8))}
        c.check(L.infur_memcpy_h2d(c.h, b["zero"], np.zeros(2, np.uint32).ctypes.data, 8))
        for name, k in (("smooth", R.smooth(h, w)), ("checkerboard", R.checkerboard(h, w))):
            c.check(L.infur_memcpy_h2d(c.h, b["plane"], k.ctypes.data, k.nbytes))
            # the counts first, then buffers of exactly the rows there are: the grid of the edge launch comes from the rows
            c.check(L.infur_outlines_dev(c.h, b["plane"], 1, h, w, 0, 0, 0, None, 0, None, 0, b["oc"]))
            nl, nv = (int(v) for v in words(c, b["oc"], 3)[:2])
            t = {key: dev_alloc(c, size) for key, size in (("lin", nl * 16), ("vin", nv * 4), ("lo", nl * 16), ("vo", nv * 4))}
            c.check(L.infur_outlines_dev(c.h, b["plane"], 1, h, w, 0, 0, 0, t["lin"], nl, t["vin"], nv, b["oc"]))
            ts = timed(c, "raster", lambda: L.infur_raster_dev(c.h, t["lin"], nl, t["vin"], nv, b["oc"], h, w, 1, 0, b["out"], b["rc"]))
            print(row(f"{name} {h}x{w}, Outlines' loops as they are", nl, nv, words(c, b["rc"], 4), ts), flush=True)
            if name == "smooth":
                c.check(L.infur_simplify_dev(c.h, t["lin"], nl, t["vin"], nv, b["oc"], h, w, 16, t["lo"], nl, t["vo"], nv, b["sc"]))
                kept = int(words(c, b["sc"], 4)[1])
                ts = timed(c, "raster", lambda: L.infur_raster_dev(c.h, t["lo"], nl, t["vo"], nv, b["sc"], h, w, 1, 0, b["out"], b["rc"]))
                print(row(f"{name} {h}x{w}, the loops at 1 px", nl, kept, words(c, b["rc"], 4), ts), flush=True)
            for d in t.values():
                L.infur_dev_free(c.h, d)
            c.check(L.infur_runs_dev(c.h, b["plane"], 1, h, w, 0, 0, None, 0, None, b["n"]))
            n = int(words(c, b["n"], 1)[0])
            runs = dev_alloc(c, n * 12)
            c.check(L.infur_runs_dev(c.h, b["plane"], 1, h, w, 0, 0, runs, n, None, b["n"]))
            ts = timed(c, "raster_runs", lambda: L.infur_raster_runs_dev(c.h, runs, n, b["n"], h, w, 1, 0, b["out"], b["rc"]))
            print(row(f"{name} {h}x{w}, Runs' records", n, "", words(c, b["rc"], 4), ts), flush=True)
            L.infur_dev_free(c.h, runs)
        ts = timed(c, "raster", lambda: L.infur_raster_dev(c.h, None, 0, None, 0, b["zero"], h, w, 1, 0, b["out"], b["rc"]))
        print(row(f"no loop at all {h}x{w}: the memset, the row pass and the finish launch", 0, 0, words(c, b["rc"], 4), ts), flush=True)
        host = R.smooth(h, w)
        for elem, plane in ((1, host), (4, host.astype(np.uint32))):
            d = dev_alloc(c, plane.nbytes)
            ts = []
            for i in range(30):
                c.synchronize()
                t0 = time.perf_counter()
                c.check(L.infur_memcpy_h2d(c.h, d, plane.ctypes.data, plane.nbytes))
                c.synchronize()
                if i >= 5:
                    ts.append((time.perf_counter() - t0) * 1e6)
            print(f"| infur_memcpy_h2d of the dense plane, {elem} byte(s) per pixel, pageable host memory (wall clock) | | | | | {statistics.median(ts):.1f} | "
                  f"{min(ts):.1f} .. {max(ts):.1f} |", flush=True)
            L.infur_dev_free(c.h, d)
        for d in b.values():
            L.infur_dev_free(c.h, d)


def fidelity():
    from infur_amd.processors import Context, polygon_fidelity

    plane = R.smooth(270, 480)
    print("\n| tolerance | polygons from | vertices in | vertices out | changed | conflict | uncovered | pixel accuracy | mIoU |\n|---|---|---|---|---|---|---|---|---|")
    with Context(device=0) as c:
        for tol16 in (8, 16, 32):
            for shared in (False, True):
                f = polygon_fidelity(c, plane, tol16, shared=shared, connectivity=4)
                print(f"| {tol16 / 16:g} px | {'Coverage (shared)' if shared else 'Simplify (loop by loop)'} | {f['vertices_in']} | {f['vertices_out']} | "
                      f"{f['changed']} | {f['conflict']} | {f['uncovered']} | {f['pixel_accuracy']:.5f} | {f['miou']:.5f} |", flush=True)


def main(argv):
    if "--fidelity" not in argv:
        measure(H, W_)
    fidelity()


if __name__ == "__main__":
    main(sys.argv[1:])
