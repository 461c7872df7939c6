#!/usr/bin/env python3
"""What Skeleton costs, on one MI355X, one context, eager launches.

``infur_skeleton_dev`` (kind plane, 2^16 table rows and counts wanted, max_rounds 0 = min(h, w) + 2) on 1080p label planes with the
``dist2`` ``infur_anchors_dev`` leaves on the device: the time of the whole call (all its launches between two HIP events; median of
25 after warm-up) --
  smooth              what a segmentation looks like: a few thousand regions, most of them tiny
  one class           one region as large as the frame: the front needs the most sub-iterations a plane of this size can ask for
  noise, 3 classes    every second pixel a region
Beside it the thin launches that did work (the first, and every one behind a launch that removed something) against those that
exited on the device word, and as yardsticks ``infur_anchors_dev`` and ``infur_split_dev`` (core 16) on the same plane and a
device-to-device copy of the plane, measured in the same sitting.
    python scripts/skeleton_rate.py             (prints a markdown table)
    python scripts/skeleton_rate.py --host      (adds the numpy reference of tests/skeleton_ref.py on the smooth plane, for scale only)
    python scripts/skeleton_rate.py --dry-run   (no device: small planes, the reference's counts, made-up times -- checks the planes
                                                 and the table code only; its numbers mean nothing)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import regions_ref as R  # noqa: E402  (the generators of the test planes)
import sieve_rate as SR  # noqa: E402  (the device helpers)
import split_rate as SPR  # noqa: E402  (the timed copy)
from infur_amd import _lib  # noqa: E402

H, W_ = 1080, 1920
K = 8  # sub-iterations per thin launch
NONE = 0xFFFFFFFF
HEAD = ("| plane | regions | max_rounds | KEPT | REMOVED | ROUNDS | ENDS | JUNCTIONS | status | thin launches: worked / exited | "
        "infur_skeleton_dev us (median of 25) | min .. max | infur_anchors_dev us | infur_split_dev us | D2D copy us |\n" + "|---" * 15 + "|")


def launches(rounds, max_rounds):
    """-> (the thin launches that did work, those that exited): launch L works when L == 1 or launch L - 1 removed something"""
    total = -(-max_rounds // K)
    worked = min(total, (rounds - 1) // K + 2 if rounds else 1)
    return worked, total - worked


def row(name, h, w, n, c, t, t_anch, t_split, t_copy):
    limit = min(h, w) + 2
    worked, exited = launches(int(c[_lib.SKELETON_ROUNDS]), limit)
    return (f"| {name} {h}x{w} | {n} | {limit} | {c[_lib.SKELETON_KEPT]} | {c[_lib.SKELETON_REMOVED]} | {c[_lib.SKELETON_ROUNDS]} | {c[_lib.SKELETON_COUNT_ENDS]} | "
            f"{c[_lib.SKELETON_COUNT_JUNCTIONS]} | {c[_lib.SKELETON_STATUS]} | {worked} / {exited} | {statistics.median(t):.1f} | {min(t):.1f} .. {max(t):.1f} | "
            f"{statistics.median(t_anch):.1f} | {statistics.median(t_split):.1f} | {statistics.median(t_copy):.1f} |")


def dry_run(h=27, w=48):
    import skeleton_ref as S

    print(HEAD)
    for name, k in SR.cases(h, w):
        labels, _, n = R.label(k, connectivity=4)
        print(row(name, h, w, n, S.skeleton(labels, None, NONE, rows=1)[2].tolist(), [30.0, 20.0, 40.0], [3.0], [9.0], [2.0]))


def host_reference(h, w):
    import skeleton_ref as S

    labels = R.label(R.smooth(h, w), connectivity=4)[0]
    t0 = time.perf_counter()
    counts = S.skeleton(labels, None, NONE, rows=1)[2]
    print(f"\nthe numpy reference on this host, smooth {h}x{w}: {time.perf_counter() - t0:.2f} s for {counts[S.ROUNDS]} sub-iterations (for scale only)")


def measure(h, w):
    from infur_amd.processors import Context

    print(HEAD)
    rows = 1 << 16
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, k in SR.cases(h, w):
            b = {key: SR.dev_alloc(c, n) for key, n in (("klass", h * w), ("labels", h * w * 4), ("n", 4), ("d2", h * w * 4), ("seg", h * w * 4), ("kind", h * w),
                                                         ("table", rows * 32), ("counts", 32))}
            c.check(L.infur_memcpy_h2d(c.h, b["klass"], k.ctypes.data, k.nbytes))
            c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, 4, 0, 0, b["labels"], None, 0, b["n"]))
            n = np.zeros(1, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, b["n"], 4))
            t_anch = SR.timed(c, "anchors", lambda: L.infur_anchors_dev(c.h, b["labels"], 4, h, w, 1, NONE, b["d2"], None, 0))
            t_split = SR.timed(c, "split", lambda: L.infur_split_dev(c.h, b["labels"], 4, b["d2"], h, w, 1, NONE, 16, 0, b["seg"], b["table"], rows, b["counts"]))
            t_copy = SPR.timed_copy(c, b["seg"], b["labels"], h * w * 4)
            t = SR.timed(c, "skeleton", lambda: L.infur_skeleton_dev(c.h, b["labels"], 4, b["d2"], h, w, 1, NONE, 0, b["kind"], b["table"], rows, b["counts"]))
            counts = np.empty(8, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, b["counts"], 32))
            print(row(name, h, w, int(n[0]), counts.tolist(), t, t_anch, t_split, t_copy), flush=True)
            for d in b.values():
                L.infur_dev_free(c.h, d)


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    measure(H, W_)
    if "--host" in argv:
        host_reference(H, W_)


if __name__ == "__main__":
    main(sys.argv[1:])
