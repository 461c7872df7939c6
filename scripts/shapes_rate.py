#!/usr/bin/env python3
"""What Shapes costs, on one MI355X, one context, eager launches.

1. ``infur_shapes_dev`` on the loops ``infur_outlines_dev`` leaves on the device for 1080p label planes (Regions, 8-connectivity,
   ``INFUR_REGION_NONE`` skipped), every output wanted and one per-value row per region: the time of the whole call (its memsets
   and launches between two HIP events; median of 25 after warm-up), beside ``infur_simplify_dev`` at tol16 = 16 on the same loops
   in the same sitting -- the yardstick: both stages walk the same vertices in the same wave-per-loop form --
     smooth              what a segmentation looks like: a few thousand regions, most of them tiny
     one class           one region, one loop of four vertices: the floor of the launches
     noise, 3 classes    every second pixel a region: the most loops a plane can have
2. PCIe-inclusive frames/s of ``FramePath.advance_shapes`` beside ``advance_regions`` on the same build in the same run, legs
   alternating, each at least a second and repeated five times, with the regions leg's own run-to-run spread.
    python scripts/shapes_rate.py [--quick]     (prints markdown tables)
    python scripts/shapes_rate.py --calls       (the first table alone)
    python scripts/shapes_rate.py --tables [--height H --width W]
                                                (no device: small planes, the reference's counts, made-up times -- checks the planes
                                                 and the table code only; its numbers mean nothing)"""
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
TOL16 = 16
NONE = 0xFFFFFFFF
LEGS = (("advance_regions (planes + labels + table)", "regions"), ("advance_shapes (table + hulls + records + rows)", "shapes"))
CALL_HEAD = ("| plane | regions | loops | vertices | longest loop | hull vertices | largest hull | infur_shapes_dev us (median of 25) | min .. max | "
             "simplified vertices | infur_simplify_dev us (median of 25) | min .. max | shapes / simplify |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|")
FRAME_HEAD = "| mode | frame | leg | frames/s (median of %d) | min .. max | vs regions |\n|---|---|---|---|---|---|"


# ---------------------------------------------------------------- planes and tables: no device needed
def cases(h, w):
    yield "smooth", R.smooth(h, w)
    yield "one class", R.single(h, w)
    yield "noise, 3 classes", R.noise(h, w, 3, seed=1)


def call_row(name, h, w, n, nl, nv, longest, shp, t_shp, simp, t_simp):
    ms, mp = statistics.median(t_shp), statistics.median(t_simp)
    return (f"| {name} {h}x{w} | {n} | {nl} | {nv} | {longest} | {shp[_lib.SHAPES_VERTICES]} | {shp[_lib.SHAPES_LARGEST]} | {ms:.1f} | "
            f"{min(t_shp):.1f} .. {max(t_shp):.1f} | {simp[_lib.SIMPLIFY_VERTICES]} | {mp:.1f} | {min(t_simp):.1f} .. {max(t_simp):.1f} | {ms / mp:.2f} |")


def frame_rows(dtype, depth, w, h, rates):
    """rates: {leg name: [frames/s per repeat]} -> the table rows of one mode and frame size"""
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    out = []
    for name, _ in LEGS:
        r = rates[name]
        out.append(f"| {dtype} r{depth} | {w}x{h} | {name} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | "
                   f"{100 * (statistics.median(r) / base - 1):+.2f} % |")
    out.append(f"| spread of the regions leg, {dtype} | {w}x{h} | | | {100 * spread:.2f} % of its median | |")
    return out


def tables(h, w):
    import outlines_ref as O
    import shapes_ref as S
    import simplify_ref as P

    print(CALL_HEAD)
    for name, k in cases(h, w):
        labels, _, n = R.label(k, connectivity=R.CONNECT_8)
        l, v, c = O.outline(labels, O.SKIP | O.CONN8, NONE)
        shp = S.shapes(l, v, c, w, rows=n)[4]
        simp = P.simplify(l, v, c, w, TOL16)[2]
        print(call_row(name, h, w, n, int(c[0]), int(c[1]), int(l[:, 1].max()), shp.tolist(), [30.0, 20.0, 40.0], simp.tolist(), [15.0, 10.0, 20.0]))
    print("\n" + FRAME_HEAD % 3)
    for dtype in ("f16hl", "f32"):
        for line in frame_rows(dtype, 50, w, h, {LEGS[0][0]: [100.0, 101.0, 99.0], LEGS[1][0]: [98.0, 99.0, 97.0]}):
            print(line)


# ---------------------------------------------------------------- the device
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


def measure_calls(h, w):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, k in cases(h, w):
            b = {key: dev_alloc(c, n) for key, n in (("klass", h * w), ("labels", h * w * 4), ("n", 4), ("oc", 12), ("hc", 16), ("pc", 16))}
            c.check(L.infur_memcpy_h2d(c.h, b["klass"], k.ctypes.data, k.nbytes))
            c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, 8, 0, 0, b["labels"], None, 0, b["n"]))
            n = np.zeros(1, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, b["n"], 4))
            n = int(n[0])
            # the counts first, then buffers of exactly the rows there are: the grids of both stages come from the rows
            c.check(L.infur_outlines_dev(c.h, b["labels"], 4, h, w, 3, NONE, 0, None, 0, None, 0, b["oc"]))
            oc = np.zeros(3, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, oc.ctypes.data, b["oc"], 12))
            nl, nv = int(oc[0]), int(oc[1])
            b.update({key: dev_alloc(c, size) for key, size in (("lin", nl * 16), ("vin", nv * 4), ("lo", nl * 16), ("vo", nv * 4), ("sh", nl * 96),
                                                                ("va", n * 96))})
            c.check(L.infur_outlines_dev(c.h, b["labels"], 4, h, w, 3, NONE, 0, b["lin"], nl, b["vin"], nv, b["oc"]))
            loops = np.zeros((nl, 4), np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, loops.ctypes.data, b["lin"], loops.nbytes))
            t_shp = timed(c, "shapes", lambda: L.infur_shapes_dev(c.h, b["lin"], nl, b["vin"], nv, b["oc"], h, w, b["lo"], nl, b["vo"], nv, b["sh"], nl,
                                                                  b["va"], n, b["hc"]))
            t_simp = timed(c, "simplify", lambda: L.infur_simplify_dev(c.h, b["lin"], nl, b["vin"], nv, b["oc"], h, w, TOL16, b["lo"], nl, b["vo"], nv,
                                                                       b["pc"]))
            shp, simp = np.empty(4, np.uint32), np.empty(4, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, shp.ctypes.data, b["hc"], 16))
            c.check(L.infur_memcpy_d2h(c.h, simp.ctypes.data, b["pc"], 16))
            print(call_row(name, h, w, n, nl, nv, int(loops[:, 1].max()), shp.tolist(), t_shp, simp.tolist(), t_simp), flush=True)
            for d in b.values():
                L.infur_dev_free(c.h, d)


class Bench:
    """the host-pointer frame paths on one context: everything they return crosses PCIe"""

    def __init__(self, dtype, depth, w, h):
        from infur_amd import weights as W
        from infur_amd.processors import Context, FramePath, Model, ModelCmd

        self.c = Context(device=0, dtype=dtype)
        Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.fp = FramePath(self.c)
        self.frame_in = W.synth_frame(h, w, index=1)

    def frame(self, leg):
        if leg == "regions":
            self.fp.advance_regions(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        else:  # the table, and the hulls, records and rows in place of the three dense planes
            self.fp.advance_shapes(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)

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
        n = max(4, int(b.leg_rate("regions", 8) * leg_s) + 1)
        rates = {name: [] for name, _ in LEGS}
        for _ in range(repeats):
            for name, leg in LEGS:
                rates[name].append(b.leg_rate(leg, n))
        for line in frame_rows(dtype, depth, w, h, rates):
            print(line, flush=True)
        b.close()


def main(argv):
    if "--tables" in argv:
        at = lambda flag, default: int(argv[argv.index(flag) + 1]) if flag in argv else default  # noqa: E731
        return tables(at("--height", 54), at("--width", 96))
    quick = (0.3, 3) if "--quick" in argv else (1.0, 5)
    measure_calls(H, W_)
    if "--calls" not in argv:
        measure_frames(*quick)


if __name__ == "__main__":
    main(sys.argv[1:])
