#!/usr/bin/env python3
"""What Compare costs, on one MI355X, one context, eager launches.

1. ``infur_compare_dev`` on 1080p planes, every output wanted: the time of the whole call (its memsets and launches between two
   HIP events; median of 25 after warm-up) --
     smooth class plane against its shift, 21 x 21 values         the dense form on what a segmentation looks like
     three-class noise against three-class noise, 3 x 3           the dense form's worst case: every run one pixel, nine LDS words
     the same noise with 64 x 65 values                           the table form under the same contention: the number that says
                                                                  whether the dense form earns its keep -- once with the default
                                                                  2^20 slots, which this plane's runs overflow (no pair is
                                                                  inserted), once with 2^22, which hold them
     two label planes of ``smooth`` (regions of it and of its shift)   the table form on what Regions produces
     the f32 against the f16hl class plane of the synthetic model, 21 x 21, with EQUAL / COMPARED
2. PCIe-inclusive frames/s of ``FramePath.advance_compare`` beside ``advance_segments`` on the same build in the same run, legs
   alternating, each at least a second and repeated five times, with the segments leg's own run-to-run spread.
3. ``--legs``: frames/s of the legs that existed before Compare (``advance_segments``, ``advance_regions``, ``advance_tracks``),
   one line per leg and mode, for comparing two builds in one sitting (--root selects the checkout whose package and library run).
    python scripts/compare_rate.py [--quick]     (prints markdown tables)
    python scripts/compare_rate.py --calls       (the first table alone)
    python scripts/compare_rate.py --legs [--quick] [--root CHECKOUT]
    python scripts/compare_rate.py --dry-run     (no device: small planes, the reference's counts, made-up times -- checks the
                                                  planes and the table code only; its numbers mean nothing)"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # --legs on another checkout of the project (its package and its library), e.g. the parent commit's
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generators of the test planes)
from infur_amd import _lib  # noqa: E402

H, W_ = 1080, 1920
NONE = 0xFFFFFFFF
LEGS = (("advance_segments (planes + statistics)", "segments"), ("advance_compare (matrix + rows + counts)", "compare"))
OLD_LEGS = ("segments", "regions", "tracks")
CALL_HEAD = ("| planes | values | form | RUNS | PAIRS | MATCHED | EQUAL / COMPARED | infur_compare_dev us (median of 25) | min .. max |\n"
             "|---|---|---|---|---|---|---|---|---|")
FRAME_HEAD = "| mode | frame | leg | frames/s (median of %d) | min .. max | vs segments |\n|---|---|---|---|---|---|"


# ---------------------------------------------------------------- planes and tables: no device needed
def shifted(plane, dy=3, dx=5):
    out = np.roll(np.roll(plane, dy, axis=0), dx, axis=1)
    out[:dy], out[:, :dx] = plane[:dy], plane[:, :dx]
    return out


def cases(h, w):
    """(name, a, b, flags, ignore_a, ignore_b, rows_a, rows_b, pair_slots)"""
    sm = R.smooth(h, w)
    n3a, n3b = R.noise(h, w, 3, seed=1), R.noise(h, w, 3, seed=2)
    yield "smooth against its shift", sm, shifted(sm), 0, 0, 0, 21, 21, 0
    yield "noise, 3 classes, twice", n3a, n3b, 0, 0, 0, 3, 3, 0
    yield "the same noise", n3a, n3b, 0, 0, 0, 64, 65, 0
    yield "the same noise, 2^22 slots", n3a, n3b, 0, 0, 0, 64, 65, 1 << 22
    (la, _, na), (lb, _, nb) = R.label(sm), R.label(shifted(sm))
    yield "label planes of smooth and its shift", la, lb, 3, NONE, NONE, na, nb, 0


def call_row(name, h, w, rows_a, rows_b, counts, ts):
    form = ("table, overflow" if counts[7] & 1 else "table") if counts[7] & 2 else "dense"
    return (f"| {name} {h}x{w} | {rows_a} x {rows_b} | {form} | {counts[6]} | {counts[4]} | {counts[5]} | {counts[1]} / {counts[0]} | "
            f"{statistics.median(ts):.1f} | {min(ts):.1f} .. {max(ts):.1f} |")


def frame_rows(dtype, depth, w, h, rates):
    """rates: {leg name: [frames/s per repeat]} -> the table rows of one mode and frame size"""
    base = statistics.median(rates[LEGS[0][0]])
    spread = (max(rates[LEGS[0][0]]) - min(rates[LEGS[0][0]])) / base
    out = []
    for name, _ in LEGS:
        r = rates[name]
        out.append(f"| {dtype} r{depth} | {w}x{h} | {name} | {statistics.median(r):.2f} | {min(r):.2f} .. {max(r):.2f} | "
                   f"{100 * (statistics.median(r) / base - 1):+.2f} % |")
    out.append(f"| spread of the segments leg, {dtype} | {w}x{h} | | | {100 * spread:.2f} % of its median | |")
    return out


def dry_run(h=54, w=96):
    import compare_ref as CR

    print(CALL_HEAD)
    for name, a, b, flags, ia, ib, ra, rb, slots in cases(h, w):
        print(call_row(name, h, w, ra, rb, CR.compare(a, b, flags, ia, ib, ra, rb, slots).counts.tolist(), [3.0, 2.0, 4.0]))
    print("\n" + FRAME_HEAD % 3)
    for dtype in ("f16hl", "f32"):
        for line in frame_rows(dtype, 50, w, h, {LEGS[0][0]: [100.0, 101.0, 99.0], LEGS[1][0]: [98.0, 99.0, 97.0]}):
            print(line)


# ---------------------------------------------------------------- the device
def dev_alloc(c, n):
    d = C.c_void_p(None)
    c.check(c.L.infur_dev_alloc(c.h, n, C.byref(d)))
    return d


def model_planes(h, w):
    """the class planes of one synthetic frame in f32 and in f16hl"""
    from infur_amd import weights as W
    from infur_amd.processors import Context, FramePath, Model, ModelCmd

    out = []
    for dtype in ("f32", "f16hl"):
        with Context(device=0, dtype=dtype) as c:
            Model(c).control(ModelCmd.LoadBlob(W.synth_blob(depth=50)))
            out.append(FramePath(c).advance_segments(W.synth_frame(h, w, index=1), 1.0, _lib.DECODE_SOFTMAX, want_conf=False, want_stats=False).klass.copy())
    return out


def measure_calls(h, w):
    from infur_amd.processors import Context

    print(CALL_HEAD)
    f32, f16hl = model_planes(h, w)
    todo = list(cases(h, w)) + [("f32 against f16hl, synthetic model", f32, f16hl, 0, 0, 0, 21, 21, 0)]
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, a, b, flags, ia, ib, ra, rb, slots in todo:
            bufs = {k: dev_alloc(c, max(n, 4)) for k, n in (("a", a.nbytes), ("b", b.nbytes), ("matrix", ra * rb * 4 if ra * rb <= 1 << 20 else 4),
                                                            ("ra", ra * 16), ("rb", rb * 16), ("counts", 32))}
            c.check(L.infur_memcpy_h2d(c.h, bufs["a"], a.ctypes.data, a.nbytes))
            c.check(L.infur_memcpy_h2d(c.h, bufs["b"], b.ctypes.data, b.nbytes))
            matrix = bufs["matrix"] if ra * rb <= 1 << 20 else None
            ts = []
            for i in range(30):
                c.check(L.infur_compare_dev(c.h, bufs["a"], a.dtype.itemsize, bufs["b"], b.dtype.itemsize, h, w, flags, ia, ib, matrix, ra, rb, bufs["ra"],
                                            bufs["rb"], bufs["counts"], slots))
                c.synchronize()
                rec = [r for r in c.profile() if r["name"] == "compare"]
                assert rec, "the call left no profile record"  # (records accumulate until the next forward: the last is this call's)
                if i >= 5:
                    ts.append(rec[-1]["ms"] * 1e3)
            counts = np.empty(8, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, bufs["counts"], 32))
            print(call_row(name, h, w, ra, rb, counts.tolist(), ts), flush=True)
            for d in bufs.values():
                L.infur_dev_free(c.h, d)


class Bench:
    """the host-pointer frame paths on one context: everything they return crosses PCIe"""

    def __init__(self, dtype, depth, w, h):
        from infur_amd import weights as W
        from infur_amd.processors import Context, FramePath, Model, ModelCmd, Tracks

        self.c = Context(device=0, dtype=dtype)
        Model(self.c).control(ModelCmd.LoadBlob(W.synth_blob(depth=depth)))
        self.fp = FramePath(self.c)
        self.tracks = Tracks(self.c)
        self.frame_in = W.synth_frame(h, w, index=1)
        self.truth = R.smooth(h, w)

    def frame(self, leg):
        if leg == "segments":
            self.fp.advance_segments(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        elif leg == "regions":
            self.fp.advance_regions(self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        elif leg == "tracks":
            self.fp.advance_tracks(self.tracks, self.frame_in, 1.0, _lib.DECODE_SOFTMAX)
        else:  # the same planes back as the segments leg, and the grade
            self.fp.advance_compare(self.frame_in, self.truth, 1.0, _lib.DECODE_SOFTMAX, want_klass=True, want_conf=True)

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
        n = max(4, int(b.leg_rate("segments", 8) * leg_s) + 1)
        rates = {name: [] for name, _ in LEGS}
        for _ in range(repeats):
            for name, leg in LEGS:
                rates[name].append(b.leg_rate(leg, n))
        for line in frame_rows(dtype, depth, w, h, rates):
            print(line, flush=True)
        b.close()


def measure_old_legs(leg_s, repeats):
    """one line per leg and mode: `legs <library> <mode> <leg> median min max`"""
    for dtype in ("f16hl", "f32"):
        b = Bench(dtype, 50, W_, H)
        for leg in OLD_LEGS:
            for _ in range(6):
                b.frame(leg)
        n = max(4, int(b.leg_rate("segments", 8) * leg_s) + 1)
        rates = {leg: [] for leg in OLD_LEGS}
        for _ in range(repeats):
            for leg in OLD_LEGS:
                rates[leg].append(b.leg_rate(leg, n))
        for leg in OLD_LEGS:
            r = rates[leg]
            print(f"legs {ROOT} {dtype} {leg} {statistics.median(r):.2f} {min(r):.2f} {max(r):.2f}", flush=True)
        b.close()


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    quick = (0.3, 3) if "--quick" in argv else (1.0, 5)
    if "--legs" in argv:
        return measure_old_legs(*quick)
    measure_calls(H, W_)
    if "--calls" not in argv:
        measure_frames(*quick)


if __name__ == "__main__":
    main(sys.argv[1:])
