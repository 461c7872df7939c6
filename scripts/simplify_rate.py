#!/usr/bin/env python3
"""What Simplify costs, on one MI355X, one context, eager launches.

1. ``infur_simplify_dev`` at ``tol16`` 11, 16 and 32 on what ``infur_outlines_dev`` left on the device for three 1080p planes --
   smooth (blobs, like a segmentation), one class, uniform noise over 21 classes (two million loops of a few vertices) -- and for
   the long-loop comb plane of the tests (130 x 2100: one loop of 136 thousand vertices, which one wave owns): the time of the
   whole call (its memset and 6 launches between two HIP events; median of 25 after warm-up), with the rows declared (the counts
   rounded up to 1024: the grids are sized by them) and the vertices and bytes before and after.
2. PCIe-inclusive frames/s of ``infur_frame_polygons`` (host pointers; counts + loop records + simplified vertices + per-class
   table come back) beside ``infur_frame_outlines`` on the same build in the same run, legs alternating, each at least a second
   and repeated five times, with the outlines leg's own run-to-run spread as the margin.
    python scripts/simplify_rate.py [--quick]    (prints markdown tables)
    python scripts/simplify_rate.py --dry-run    (no device: small planes, the reference's counts, made-up times -- checks the
                                                  planes and the table code only; its numbers mean nothing)"""
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
import simplify_ref as S  # noqa: E402
from infur_amd import _lib  # noqa: E402

H, W_ = 1080, 1920
TOLS = (11, 16, 32)
LEGS = (("infur_frame_outlines (counts + loops + vertices + stats)", "outlines"), ("infur_frame_polygons, tol16 16 (the same, simplified)", "polygons"))
CALL_HEAD = ("| plane | tol16 | loops | vertices | vertices kept | degenerate loops | bytes before | bytes after | rows declared (loops, vertices) | "
             "infur_simplify_dev us (median of 25) | min .. max |\n|---|---|---|---|---|---|---|---|---|---|---|")
FRAME_HEAD = "| leg | mode | frame | frames/s (median of %d) | min .. max | vs outlines | bytes to the host per frame |\n|---|---|---|---|---|---|---|"


# ---------------------------------------------------------------- planes and tables: no device needed
def planes(h, w, comb_shape):
    """-> (name, plane, outlines flags, skip value)"""
    yield f"smooth {h}x{w}", R.smooth(h, w), 0, 0
    yield f"one class {h}x{w}", R.single(h, w), 0, 0
    yield f"noise, 21 classes {h}x{w}", R.noise(h, w, 21), 0, 0
    yield "comb %dx%d" % comb_shape, S.comb(*comb_shape), _lib.OUTLINES_SKIP, 0


def polygon_bytes(n_loops, n_vertices):
    return 16 * n_loops + 4 * n_vertices


def call_row(name, tol16, counts_in, counts_out, rows, ts):
    nl, nv = int(counts_in[0]), int(counts_in[1])
    return (f"| {name} | {tol16} | {nl} | {nv} | {int(counts_out[1])} | {int(counts_out[2])} | {polygon_bytes(nl, nv)} | {polygon_bytes(nl, int(counts_out[1]))} | "
            f"{rows[0]}, {rows[1]} | {statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |")


def frame_rows(dtype, depth, w, h, k, rates, sizes):
    """rates: {leg name: [frames/s per repeat]}, sizes: {leg: (n_loops, n_vertices)} -> the table rows of one mode and frame size"""
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    out = []
    for name, leg in LEGS:
        r = rates[name]
        out.append(f"| {name} | {dtype} r{depth} | {w}x{h} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | "
                   f"{100 * (statistics.median(r) / base - 1):+.2f} % | {16 + polygon_bytes(*sizes[leg]) + k * _lib.STAT_WORDS * 8} |")
    out.append(f"| spread of the outlines leg | {dtype} r{depth} | {w}x{h} | | {100 * spread:.2f} % of its median | | |")
    return out


def dry_run(h=54, w=96):
    import outlines_ref as O

    print(CALL_HEAD)
    for name, plane, flags, skip in planes(h, w, (20, 100)):
        l, v, c = O.outline(plane, flags, skip)
        for tol16 in TOLS:
            print(call_row(name, tol16, c, S.simplify(l, v, c, plane.shape[1], tol16)[2], (len(l), len(v)), [3.0, 2.0, 4.0]))
    print("\n" + FRAME_HEAD % 3)
    l, v, c = O.outline(R.smooth(h, w))
    kept = S.simplify(l, v, c, w, 16)[2]
    sizes = {"outlines": (int(c[0]), int(c[1])), "polygons": (int(kept[0]), int(kept[1]))}
    for line in frame_rows("f32", 50, w, h, 21, {LEGS[0][0]: [100.0, 101.0, 99.0], LEGS[1][0]: [98.0, 99.0, 97.0]}, sizes):
        print(line)


# ---------------------------------------------------------------- the device
def dev_alloc(c, n):
    d = C.c_void_p(None)
    c.check(c.L.infur_dev_alloc(c.h, max(n, 4), C.byref(d)))
    return d


def measure_calls(h, w):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, plane, flags, skip in planes(h, w, (130, 2100)):
            ph, pw = plane.shape
            N = ph * pw
            bufs = {k: dev_alloc(c, n) for k, n in (("plane", N), ("loops", N * 16), ("vertices", N * 16), ("counts", 12), ("lout", N * 16), ("vout", N * 16),
                                                    ("cout", 16))}
            c.check(L.infur_memcpy_h2d(c.h, bufs["plane"], plane.ctypes.data, plane.nbytes))
            c.check(L.infur_outlines_dev(c.h, bufs["plane"], 1, ph, pw, flags, skip, 0, bufs["loops"], N, bufs["vertices"], 4 * N, bufs["counts"]))
            counts = np.zeros(3, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, bufs["counts"], 12))
            rows = tuple((int(n) + 1023) // 1024 * 1024 for n in counts[:2])  # what a caller that knows its scenes gives Outlines
            for tol16 in TOLS:
                ts = []
                for i in range(30):
                    c.check(L.infur_simplify_dev(c.h, bufs["loops"], rows[0], bufs["vertices"], rows[1], bufs["counts"], ph, pw, tol16, bufs["lout"], rows[0],
                                                 bufs["vout"], rows[1], bufs["cout"]))
                    c.synchronize()
                    rec = [r for r in c.profile() if r["kernel"] == "simplify"]
                    assert rec, "the call left no profile record"  # (records accumulate until the next forward: the last is this call's)
                    if i >= 5:
                        ts.append(rec[-1]["ms"] * 1e3)
                cout = np.zeros(4, np.uint32)
                c.check(L.infur_memcpy_d2h(c.h, cout.ctypes.data, bufs["cout"], 16))
                assert cout[3] == 0
                print(call_row(name, tol16, counts, cout, rows, ts), flush=True)
            for d in bufs.values():
                L.infur_dev_free(c.h, d)


class Bench:
    """the two host-pointer frame calls on one context: everything they return crosses PCIe"""

    def __init__(self, dtype, depth, w, h):
        from infur_amd import weights as W
        from infur_amd.processors import Context, Model, ModelCmd

        self.c = Context(device=0, dtype=dtype)
        m = Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.k = m.get_info().num_classes
        self.w, self.h = w, h
        self.frame_in = W.synth_frame(h, w, index=1)
        self.stats = np.zeros((self.k, _lib.STAT_WORDS), np.uint64)
        self.loops = np.empty((w * h, _lib.LOOP_WORDS), np.uint32)
        self.vertices = np.empty(4 * w * h, np.uint32)
        self.counts = {"outlines": np.zeros(3, np.uint32), "polygons": np.zeros(4, np.uint32)}
        self.ow, self.oh = C.c_uint32(0), C.c_uint32(0)

    def frame(self, leg):
        L, hd, w, h = self.c.L, self.c.h, self.w, self.h
        tail = (self.loops.ctypes.data, w * h, self.vertices.ctypes.data, 4 * w * h, self.counts[leg].ctypes.data, self.stats.ctypes.data, self.k, None,
                C.byref(self.ow), C.byref(self.oh))
        if leg == "outlines":
            rc = L.infur_frame_outlines(hd, self.frame_in.ctypes.data, w, h, 1.0, 0, _lib.DECODE_SOFTMAX, 0, 0, 0, *tail)
        else:
            rc = L.infur_frame_polygons(hd, self.frame_in.ctypes.data, w, h, 1.0, 0, _lib.DECODE_SOFTMAX, 0, 0, 0, 16, *tail)
        self.c.check(rc)

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
        n = max(4, int(b.leg_rate("outlines", 8) * leg_s) + 1)
        rates = {name: [] for name, _ in LEGS}
        for _ in range(repeats):
            for name, leg in LEGS:
                rates[name].append(b.leg_rate(leg, n))
        sizes = {leg: (int(b.counts[leg][0]), int(b.counts[leg][1])) for _, leg in LEGS}
        for line in frame_rows(dtype, depth, w, h, b.k, rates, sizes):
            print(line, flush=True)
        b.close()


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    timing = (0.3, 3) if "--quick" in argv else (1.0, 5)
    measure_calls(H, W_)
    measure_frames(*timing)


if __name__ == "__main__":
    main(sys.argv[1:])
