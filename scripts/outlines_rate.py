#!/usr/bin/env python3
"""What Outlines costs, on one MI355X, one context, eager launches.

1. ``infur_outlines_dev`` on 1080p planes -- smooth (blobs, like a segmentation), one class, uniform noise over 21 classes (the
   adversarial case: nearly every side of every pixel is an edge) -- as class bytes and as u32 label planes, with the default
   edge capacity (four per pixel), and the smooth plane again with ``max_edges`` = 1 Mi: the time of the whole call (its 9 + K
   launches between two HIP events; median of 25 after warm-up) beside a device-to-device copy of the plane, with the number of
   edges, loops and vertices.
2. PCIe-inclusive frames/s of ``infur_frame_outlines`` (host pointers; counts + loop records + vertices + per-class table come
   back) beside ``infur_frame_segments`` (class plane + per-class table) on the same build in the same run, legs alternating,
   each at least a second and repeated five times, with the segments leg's own run-to-run spread.
    python scripts/outlines_rate.py [--quick]           (prints markdown tables)
    python scripts/outlines_rate.py --segments-only     (the second table with the segments leg alone: its spread on any build)
    python scripts/outlines_rate.py --dry-run           (no device: small planes, the reference's counts, made-up times -- checks
                                                         the planes and the table code only; its numbers mean nothing)"""
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
MI = 1 << 20
LEGS = (("infur_frame_segments (class plane + stats)", "segments"), ("infur_frame_outlines (counts + loops + vertices + stats)", "outlines"))
CALL_HEAD = ("| plane | element | max_edges | edges | loops | vertices | rounds | infur_outlines_dev us (median of 25) | min .. max | D2D copy of the plane, us |\n"
             "|---|---|---|---|---|---|---|---|---|---|")
FRAME_HEAD = "| mode | frame | leg | frames/s (median of %d) | min .. max | vs segments | bytes to the host per frame |\n|---|---|---|---|---|---|---|"


# ---------------------------------------------------------------- planes and tables: no device needed
def planes(h, w):
    """-> (name, elem_bytes, max_edges, plane): each family as class bytes and as a u32 label plane (its connected regions; for
    the noise plane, whose labelling on the CPU takes minutes, its classes spread over the u32 range), with the default capacity;
    the smooth class plane once more with room for 1 Mi edges"""
    for name, klass in (("smooth", R.smooth(h, w)), ("one class", R.single(h, w)), ("noise, 21 classes", R.noise(h, w, 21))):
        yield name, 1, 0, klass
        yield name, 4, 0, np.ascontiguousarray(R.label(klass, None, 8)[0] if not name.startswith("noise") else klass.astype(np.uint32) * 0x01010101)
        if name == "smooth":
            yield name, 1, MI, klass


def rounds(h, w, max_edges):
    cap = max_edges if 0 < max_edges < 4 * h * w else 4 * h * w
    return max(0, (cap - 1).bit_length())


def call_row(name, h, w, elem, max_edges, counts, ts, copy_us):
    n_loops, n_vertices, n_edges = counts
    return (f"| {name} {h}x{w} | {'u8 class' if elem == 1 else 'u32 label'} | {max_edges} | {n_edges} | {n_loops} | {n_vertices} | {rounds(h, w, max_edges)} | "
            f"{statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} | {copy_us:.1f} |")


def bytes_to_host(leg, w, h, k, counts):
    stats = k * _lib.STAT_WORDS * 8
    return w * h + stats if leg == "segments" else 12 + counts[0] * 16 + counts[1] * 4 + stats


def frame_rows(dtype, depth, w, h, k, rates, counts, legs=LEGS):
    """rates: {leg name: [frames/s per repeat]} -> the table rows of one mode and frame size"""
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    out = []
    for name, leg in legs:
        r = rates[name]
        out.append(f"| {dtype} r{depth} | {w}x{h} | {name} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | "
                   f"{100 * (statistics.median(r) / base - 1):+.2f} % | {bytes_to_host(leg, w, h, k, counts)} |")
    out.append(f"| {dtype} r{depth} | {w}x{h} | spread of the segments leg | | {100 * spread:.2f} % of its median | | "
               f"({counts[0]} loops, {counts[1]} vertices, {counts[2]} edges in the frame) |")
    return out


def dry_run(h=54, w=96):
    import outlines_ref as O

    print(CALL_HEAD)
    for name, elem, max_edges, plane in planes(h, w):
        assert plane.shape == (h, w) and plane.dtype.itemsize == elem
        print(call_row(name, h, w, elem, max_edges, O.outline(plane)[2].tolist(), [3.0, 2.0, 4.0], 1.0))
    print("\n" + FRAME_HEAD % 3)
    counts = O.outline(R.smooth(h, w))[2].tolist()
    for line in frame_rows("f32", 50, w, h, 21, {LEGS[0][0]: [100.0, 101.0, 99.0], LEGS[1][0]: [98.0, 99.0, 97.0]}, counts):
        print(line)


# ---------------------------------------------------------------- the device
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


def measure_calls(h, w):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    with Context(device=0, profile=True) as c:
        L, N = c.L, h * w
        bufs = {name: dev_alloc(c, n) for name, n in (("plane", N * 4), ("loops", N * 16), ("vertices", N * 16), ("counts", 12))}
        copy_us = {1: d2d_copy_us(c, N), 4: d2d_copy_us(c, N * 4)}
        for name, elem, max_edges, plane in planes(h, w):
            c.check(L.infur_memcpy_h2d(c.h, bufs["plane"], plane.ctypes.data, plane.nbytes))
            ts = []
            for i in range(30):
                c.check(L.infur_outlines_dev(c.h, bufs["plane"], elem, h, w, 0, 0, max_edges, bufs["loops"], N, bufs["vertices"], 4 * N, bufs["counts"]))
                c.synchronize()
                rec = [r for r in c.profile() if r["kernel"] == "outlines"]
                assert rec, "the call left no profile record"  # (records accumulate until the next forward: the last is this call's)
                if i >= 5:
                    ts.append(rec[-1]["ms"] * 1e3)
            counts = np.zeros(3, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, bufs["counts"], 12))
            print(call_row(name, h, w, elem, max_edges, counts.tolist(), ts, copy_us[elem]), flush=True)
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
        self.klass = np.empty((h, w), np.uint8)
        self.stats = np.zeros((self.k, _lib.STAT_WORDS), np.uint64)
        self.loops = np.empty((w * h, _lib.LOOP_WORDS), np.uint32)
        self.vertices = np.empty(4 * w * h, np.uint32)
        self.counts = np.zeros(3, np.uint32)
        self.ow, self.oh = C.c_uint32(0), C.c_uint32(0)

    def frame(self, leg):
        L, hd, w, h = self.c.L, self.c.h, self.w, self.h
        if leg == "segments":
            rc = L.infur_frame_segments(hd, self.frame_in.ctypes.data, w, h, 1.0, 0, _lib.DECODE_SOFTMAX, self.klass.ctypes.data, None, w * h,
                                        self.stats.ctypes.data, self.k, None, 0, None, C.byref(self.ow), C.byref(self.oh))
        else:
            rc = L.infur_frame_outlines(hd, self.frame_in.ctypes.data, w, h, 1.0, 0, _lib.DECODE_SOFTMAX, 0, 0, 0, self.loops.ctypes.data, w * h,
                                        self.vertices.ctypes.data, 4 * w * h, self.counts.ctypes.data, self.stats.ctypes.data, self.k, None,
                                        C.byref(self.ow), C.byref(self.oh))
        self.c.check(rc)

    def leg_rate(self, leg, n):
        self.c.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.frame(leg)  # (the host-pointer calls synchronise themselves)
        return n / (time.perf_counter() - t0)

    def close(self):
        self.c.close()


def measure_frames(leg_s, repeats, legs=LEGS):
    print("\n" + FRAME_HEAD % repeats)
    for dtype, depth, w, h in (("f16hl", 50, W_, H), ("f32", 50, W_, H), ("f16hl", 50, 640, 480), ("f32", 50, 640, 480)):
        b = Bench(dtype, depth, w, h)
        for _, leg in legs:  # warm every leg (arena, tile configurations, scratch)
            for _ in range(6):
                b.frame(leg)
        n = max(4, int(b.leg_rate("segments", 8) * leg_s) + 1)
        rates = {name: [] for name, _ in legs}
        for _ in range(repeats):
            for name, leg in legs:
                rates[name].append(b.leg_rate(leg, n))
        for line in frame_rows(dtype, depth, w, h, b.k, rates, b.counts.tolist(), legs):
            print(line, flush=True)
        b.close()


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    timing = (0.3, 3) if "--quick" in argv else (1.0, 5)
    if "--segments-only" in argv:
        return measure_frames(*timing, legs=LEGS[:1])
    measure_calls(H, W_)
    measure_frames(*timing)


if __name__ == "__main__":
    main(sys.argv[1:])
