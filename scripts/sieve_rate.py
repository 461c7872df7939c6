#!/usr/bin/env python3
"""What Adjacency and Sieve cost, on one MI355X, one context, eager launches.

1. ``infur_adjacency_dev`` of the label plane and ``infur_sieve_dev`` (min_pixels 64, the default rounds and slots) on what
   ``infur_regions_dev`` leaves on the device for 1080p class planes, every output wanted: the time of the whole call (its memsets
   and launches between two HIP events; median of 25 after warm-up), at both connectivities --
     smooth              what a segmentation looks like: a few thousand regions, most of them tiny
     one class           one region, no border: the floor of the two plane passes
     noise, 3 classes    every second pixel a region: the runs overflow the default 2^20 slots, nothing is inserted
2. PCIe-inclusive frames/s of ``FramePath.advance_sieve`` beside ``advance_regions`` on the same build in the same run (the same
   planes and table coming back), legs alternating, each at least a second and repeated five times, with the regions leg's own
   run-to-run spread.
    python scripts/sieve_rate.py [--quick]     (prints markdown tables)
    python scripts/sieve_rate.py --calls       (the first table alone)
    python scripts/sieve_rate.py --dry-run     (no device: small planes, the reference's counts, made-up times -- checks the planes
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
MIN_PIXELS = 64
LEGS = (("advance_regions (planes + labels + table)", "regions"), ("advance_sieve (the same of the cleaned plane + counts)", "sieve"))
CALL_HEAD = ("| plane | connectivity | regions | RUNS | PAIRS | adjacency status | infur_adjacency_dev us (median of 25) | min .. max | SMALL | ABSORBED | ROUNDS | "
             "PIXELS_CHANGED | sieve status | infur_sieve_dev us (median of 25) | min .. max |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
FRAME_HEAD = "| mode | frame | leg | frames/s (median of %d) | min .. max | vs regions |\n|---|---|---|---|---|---|"


# ---------------------------------------------------------------- planes and tables: no device needed
def cases(h, w):
    yield "smooth", R.smooth(h, w)
    yield "one class", R.single(h, w)
    yield "noise, 3 classes", R.noise(h, w, 3, seed=1)


def call_row(name, h, w, conn, n, adj, t_adj, sv, t_sv):
    return (f"| {name} {h}x{w} | {conn} | {n} | {adj[_lib.ADJ_RUNS]} | {adj[_lib.ADJ_PAIRS]} | {adj[_lib.ADJ_STATUS]} | {statistics.median(t_adj):.1f} | "
            f"{min(t_adj):.1f} .. {max(t_adj):.1f} | {sv[_lib.SIEVE_SMALL]} | {sv[_lib.SIEVE_ABSORBED]} | {sv[_lib.SIEVE_ROUNDS]} | "
            f"{sv[_lib.SIEVE_PIXELS_CHANGED]} | {sv[_lib.SIEVE_STATUS]} | {statistics.median(t_sv):.1f} | {min(t_sv):.1f} .. {max(t_sv):.1f} |")


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


def dry_run(h=54, w=96):
    import sieve_ref as S

    print(CALL_HEAD)
    for name, k in cases(h, w):
        for conn in (4, 8):
            labels, table, n = R.label(k, connectivity=conn)
            adj = S.adjacency(labels, n, pair_slots=1024)
            sv = S.sieve(k, labels, table, n, min_pixels=MIN_PIXELS, pair_slots=1024)
            print(call_row(name, h, w, conn, n, adj.counts.tolist(), [3.0, 2.0, 4.0], sv.counts.tolist(), [30.0, 20.0, 40.0]))
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
            for conn in (4, 8):
                b = {key: dev_alloc(c, n) for key, n in (("klass", h * w), ("labels", h * w * 4), ("n", 4), ("out", h * w), ("ac", 32), ("sc", 32))}
                c.check(L.infur_memcpy_h2d(c.h, b["klass"], k.ctypes.data, k.nbytes))
                c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, conn, 0, 0, b["labels"], None, 0, b["n"]))
                n = np.zeros(1, np.uint32)
                c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, b["n"], 4))
                n = int(n[0])
                pair_rows = 1 << 17
                b.update({key: dev_alloc(c, size) for key, size in (("table", n * 80), ("pairs", pair_rows * 16), ("arows", n * 16), ("srows", n * 16))})
                c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, conn, 0, 0, b["labels"], b["table"], n, b["n"]))
                t_adj = timed(c, "adjacency", lambda: L.infur_adjacency_dev(c.h, b["labels"], 4, h, w, 0, 0, n, b["pairs"], pair_rows, b["arows"], b["ac"], 0))
                t_sv = timed(c, "sieve", lambda: L.infur_sieve_dev(c.h, b["klass"], b["labels"], b["table"], n, b["n"], h, w, MIN_PIXELS, 0, 0, b["out"],
                                                                   b["srows"], b["sc"]))
                adj, sv = np.empty(8, np.uint32), np.empty(8, np.uint32)
                c.check(L.infur_memcpy_d2h(c.h, adj.ctypes.data, b["ac"], 32))
                c.check(L.infur_memcpy_d2h(c.h, sv.ctypes.data, b["sc"], 32))
                print(call_row(name, h, w, conn, n, adj.tolist(), t_adj, sv.tolist(), t_sv), flush=True)
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
        else:  # the same planes, labels and table back, of the cleaned plane, and the counts
            self.fp.advance_sieve(self.frame_in, MIN_PIXELS, 1.0, _lib.DECODE_SOFTMAX)

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
    if "--dry-run" in argv:
        return dry_run()
    quick = (0.3, 3) if "--quick" in argv else (1.0, 5)
    measure_calls(H, W_)
    if "--calls" not in argv:
        measure_frames(*quick)


if __name__ == "__main__":
    main(sys.argv[1:])
