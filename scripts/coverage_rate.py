#!/usr/bin/env python3
"""What Coverage costs beside Simplify, on one MI355X, one context, eager launches, the same build, the same run.

1. ``infur_coverage_dev`` against ``infur_simplify_dev`` at ``tol16`` 11, 16 and 32 on what ``infur_outlines_dev`` left on the
   device for the four planes of scripts/simplify_rate.py (1080p smooth, one class, noise over 21 classes, and the long-loop comb
   130 x 2100): the time of each whole call between two HIP events, the two calls alternating, median of 25 after warm-up, with
   the vertices kept by each, n_aug, n_arcs and the bytes before and after.  The rows declared are the counts rounded up to
   1024, aug_rows is n_aug rounded up likewise.
2. PCIe-inclusive frames/s of ``infur_frame_coverage`` beside ``infur_frame_polygons`` and ``infur_frame_outlines``, legs
   alternating, each at least a second and repeated five times, with the outlines leg's own run-to-run spread as the margin.
    python scripts/coverage_rate.py [--quick]    (prints markdown tables)
    python scripts/coverage_rate.py --dry-run    (no device: small planes, the references' counts, made-up times -- checks the
                                                  planes and the table code only; its numbers mean nothing)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import simplify_rate as SR  # noqa: E402  (its planes, its device helpers)
from infur_amd import _lib  # noqa: E402

TOLS = SR.TOLS
LEGS = (("infur_frame_outlines (counts + loops + vertices + stats)", "outlines"), ("infur_frame_polygons, tol16 16 (loop by loop)", "polygons"),
        ("infur_frame_coverage, tol16 16 (shared borders once)", "coverage"))
CALL_HEAD = ("| plane | tol16 | loops | vertices | n_aug | n_arcs | kept by Simplify | kept by Coverage | bytes before | bytes after (Coverage) | "
             "infur_simplify_dev us (median of 25) | min .. max | infur_coverage_dev us (median of 25) | min .. max | ratio |\n"
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
FRAME_HEAD = "| leg | mode | frame | frames/s (median of %d) | min .. max | vs outlines | bytes to the host per frame |\n|---|---|---|---|---|---|---|"


def call_row(name, tol16, counts_in, simp, cov, ts_s, ts_c):
    nl, nv = int(counts_in[0]), int(counts_in[1])
    ms, mc = statistics.median(ts_s), statistics.median(ts_c)
    return (f"| {name} | {tol16} | {nl} | {nv} | {int(cov[4])} | {int(cov[5])} | {int(simp[1])} | {int(cov[1])} | {SR.polygon_bytes(nl, nv)} | "
            f"{SR.polygon_bytes(nl, int(cov[1]))} | {ms:.1f} | {min(ts_s):.1f} .. {max(ts_s):.1f} | {mc:.1f} | {min(ts_c):.1f} .. {max(ts_c):.1f} | {mc / ms:.2f} |")


def frame_rows(dtype, depth, w, h, k, rates, sizes):
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    out = []
    for name, leg in LEGS:
        r = rates[name]
        out.append(f"| {name} | {dtype} r{depth} | {w}x{h} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | "
                   f"{100 * (statistics.median(r) / base - 1):+.2f} % | {16 + SR.polygon_bytes(*sizes[leg]) + k * _lib.STAT_WORDS * 8} |")
    out.append(f"| spread of the outlines leg | {dtype} r{depth} | {w}x{h} | | {100 * spread:.2f} % of its median | | |")
    return out


def dry_run(h=54, w=96):
    import coverage_ref as V
    import outlines_ref as O
    import simplify_ref as S

    print(CALL_HEAD)
    for name, plane, flags, skip in SR.planes(h, w, (20, 100)):
        l, v, c = O.outline(plane, flags, skip)
        for tol16 in TOLS:
            print(call_row(name, tol16, c, S.simplify(l, v, c, plane.shape[1], tol16)[2], V.coverage(plane, l, v, c, tol16, flags & 1, skip)[2], [3.0, 2.0, 4.0],
                           [5.0, 4.0, 6.0]))
    print("\n" + FRAME_HEAD % 3)
    from regions_ref import smooth

    plane = smooth(h, w)
    l, v, c = O.outline(plane)
    ks, kc = S.simplify(l, v, c, w, 16)[2], V.coverage(plane, l, v, c, 16)[2]
    sizes = {"outlines": (int(c[0]), int(c[1])), "polygons": (int(ks[0]), int(ks[1])), "coverage": (int(kc[0]), int(kc[1]))}
    for line in frame_rows("f32", 50, w, h, 21, {LEGS[0][0]: [100.0, 101.0, 99.0], LEGS[1][0]: [98.0, 99.0, 97.0], LEGS[2][0]: [97.0, 98.0, 96.0]}, sizes):
        print(line)


def last_ms(c, kernel):
    rec = [r for r in c.profile() if r["kernel"] == kernel]
    assert rec, f"the {kernel} call left no profile record"  # (records accumulate until the next forward: the last is this call's)
    return rec[-1]["ms"] * 1e3


def measure_calls(h, w):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, plane, flags, skip in SR.planes(h, w, (130, 2100)):
            ph, pw = plane.shape
            N = ph * pw
            bufs = {k: SR.dev_alloc(c, n) for k, n in (("plane", N), ("loops", N * 16), ("vertices", N * 16), ("counts", 12), ("lout", N * 16),
                                                       ("vout", N * 16 + (ph + 1) * (pw + 1) * 4), ("cout", 24))}
            c.check(L.infur_memcpy_h2d(c.h, bufs["plane"], plane.ctypes.data, plane.nbytes))
            c.check(L.infur_outlines_dev(c.h, bufs["plane"], 1, ph, pw, flags, skip, 0, bufs["loops"], N, bufs["vertices"], 4 * N, bufs["counts"]))
            counts = np.zeros(3, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, bufs["counts"], 12))
            rows = tuple((int(n) + 1023) // 1024 * 1024 for n in counts[:2])  # what a caller that knows its scenes gives Outlines
            cov = np.zeros(6, np.uint32)

            def coverage(tol16, aug_rows):
                c.check(L.infur_coverage_dev(c.h, bufs["plane"], 1, ph, pw, flags & 1, skip, bufs["loops"], rows[0], bufs["vertices"], rows[1], bufs["counts"],
                                             tol16, aug_rows, bufs["lout"], rows[0], bufs["vout"], 4 * N + (ph + 1) * (pw + 1), bufs["cout"]))
                c.synchronize()

            coverage(16, 0)  # the worst-case capacity once, for n_aug
            c.check(L.infur_memcpy_d2h(c.h, cov.ctypes.data, bufs["cout"], 24))
            aug_rows = (int(cov[4]) + 1023) // 1024 * 1024
            for tol16 in TOLS:
                ts_s, ts_c = [], []
                simp = np.zeros(4, np.uint32)
                for i in range(30):  # the two calls alternate
                    c.check(L.infur_simplify_dev(c.h, bufs["loops"], rows[0], bufs["vertices"], rows[1], bufs["counts"], ph, pw, tol16, bufs["lout"], rows[0],
                                                 bufs["vout"], rows[1], bufs["cout"]))
                    c.synchronize()
                    t = last_ms(c, "simplify")
                    if i == 29:
                        c.check(L.infur_memcpy_d2h(c.h, simp.ctypes.data, bufs["cout"], 16))
                    coverage(tol16, aug_rows)
                    if i >= 5:
                        ts_s.append(t)
                        ts_c.append(last_ms(c, "coverage"))
                c.check(L.infur_memcpy_d2h(c.h, cov.ctypes.data, bufs["cout"], 24))
                assert simp[3] == 0 and cov[3] == 0
                print(call_row(name, tol16, counts, simp, cov, ts_s, ts_c), flush=True)
            for d in bufs.values():
                L.infur_dev_free(c.h, d)


class Bench(SR.Bench):
    """the three host-pointer frame calls on one context: everything they return crosses PCIe"""

    def __init__(self, dtype, depth, w, h):
        super().__init__(dtype, depth, w, h)
        self.vertices = np.empty(4 * w * h + (w + 1) * (h + 1), np.uint32)
        self.counts["coverage"] = np.zeros(6, np.uint32)

    def frame(self, leg):
        if leg != "coverage":
            return super().frame(leg)
        L, hd, w, h = self.c.L, self.c.h, self.w, self.h
        self.c.check(L.infur_frame_coverage(hd, self.frame_in.ctypes.data, w, h, 1.0, 0, _lib.DECODE_SOFTMAX, 0, 0, 0, 16, self.loops.ctypes.data, w * h,
                                            self.vertices.ctypes.data, len(self.vertices), self.counts[leg].ctypes.data, self.stats.ctypes.data, self.k, None,
                                            C.byref(self.ow), C.byref(self.oh)))


def measure_frames(leg_s, repeats):
    print("\n" + FRAME_HEAD % repeats)
    for dtype, depth, w, h in (("f16hl", 50, SR.W_, SR.H), ("f32", 50, SR.W_, SR.H)):
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
    measure_calls(SR.H, SR.W_)
    measure_frames(*timing)


if __name__ == "__main__":
    main(sys.argv[1:])
