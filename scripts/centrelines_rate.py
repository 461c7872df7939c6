#!/usr/bin/env python3
"""What Centrelines costs, on one MI355X, one context, eager launches.

``infur_centrelines_dev`` (2^20 records, 2^22 vertices and the counts wanted, max_links = h * w) on 1080p label planes with the kind
plane ``infur_skeleton_dev`` and the ``dist2`` ``infur_anchors_dev`` leave on the device: the time of the whole call (all its launches
between two HIP events; median of 25 after warm-up) --
  smooth              what a segmentation looks like: a few thousand regions, most of them tiny
  one class           one region as large as the frame: a single centreline
  noise, 3 classes    every second pixel a region
Beside it the rounds of the list ranking that worked (the longest branch decides) of those launched, and as yardsticks
``infur_skeleton_dev`` and ``infur_outlines_dev`` on the same plane and a device-to-device copy of the plane, measured in the same
sitting.
    python scripts/centrelines_rate.py             (prints a markdown table)
    python scripts/centrelines_rate.py --dry-run   (no device: small planes, the reference's counts, made-up times -- checks the planes
                                                    and the table code only; its numbers mean nothing)"""
import os
import statistics
import sys

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
NONE = 0xFFFFFFFF
HEAD = ("| plane | regions | BRANCHES | VERTICES | LINKS | NODES | ENDS | RINGS | status | longest branch (links) | rounds: worked / launched | "
        "infur_centrelines_dev us (median of 25) | min .. max | infur_skeleton_dev us | infur_outlines_dev us | D2D copy us |\n" + "|---" * 16 + "|")


def rounds(longest, max_links):
    """-> (the rounds that worked, those launched): a chain of n darts is finished after ceil(log2 n) rounds, one more meets only
    finished darts, and the rounds behind that one exit"""
    launched = max(1, (2 * max_links - 1).bit_length()) + 1
    return min(launched, max(1, (max(longest, 1) - 1).bit_length() + 1)), launched


def row(name, h, w, n, c, longest, max_links, t, t_skel, t_outl, t_copy):
    worked, launched = rounds(longest, max_links)
    return (f"| {name} {h}x{w} | {n} | {c[_lib.CENTRELINES_BRANCHES]} | {c[_lib.CENTRELINES_VERTICES]} | {c[_lib.CENTRELINES_LINKS]} | {c[_lib.CENTRELINES_NODES]} | "
            f"{c[_lib.CENTRELINES_ENDS]} | {c[_lib.CENTRELINES_RINGS]} | {c[_lib.CENTRELINES_STATUS]} | {longest} | {worked} / {launched} | {statistics.median(t):.1f} | "
            f"{min(t):.1f} .. {max(t):.1f} | {statistics.median(t_skel):.1f} | {statistics.median(t_outl):.1f} | {statistics.median(t_copy):.1f} |")


def dry_run(h=27, w=48):
    import centrelines_ref as CL
    import skeleton_ref as S

    print(HEAD)
    for name, k in SR.cases(h, w):
        labels, _, n = R.label(k, connectivity=4)
        rec, _, counts = CL.centrelines(labels, S.skeleton(labels, None, NONE, rows=1)[0], None, NONE)
        longest = int((rec[:, CL.ORTHO] + rec[:, CL.DIAG]).max()) if len(rec) else 0
        print(row(name, h, w, n, counts.tolist(), longest, h * w, [30.0, 20.0, 40.0], [3.0], [9.0], [2.0]))


def measure(h, w):
    from infur_amd.processors import Context

    print(HEAD)
    rows, vrows, max_links = 1 << 20, 1 << 22, h * w
    with Context(device=0, profile=True) as c:
        L = c.L
        for name, k in SR.cases(h, w):
            b = {key: SR.dev_alloc(c, n) for key, n in (("klass", h * w), ("labels", h * w * 4), ("n", 4), ("d2", h * w * 4), ("copy", h * w * 4), ("kind", h * w),
                                                         ("records", rows * 32), ("vertices", vrows * 4), ("counts", 32))}
            c.check(L.infur_memcpy_h2d(c.h, b["klass"], k.ctypes.data, k.nbytes))
            c.check(L.infur_regions_dev(c.h, b["klass"], None, h, w, 4, 0, 0, b["labels"], None, 0, b["n"]))
            n = np.zeros(1, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, n.ctypes.data, b["n"], 4))
            c.check(L.infur_anchors_dev(c.h, b["labels"], 4, h, w, 1, NONE, b["d2"], None, 0))
            t_skel = SR.timed(c, "skeleton", lambda: L.infur_skeleton_dev(c.h, b["labels"], 4, b["d2"], h, w, 1, NONE, 0, b["kind"], None, 0, b["counts"]))
            t_outl = SR.timed(c, "outlines", lambda: L.infur_outlines_dev(c.h, b["labels"], 4, h, w, 1, NONE, 0, b["records"], rows, b["vertices"], vrows, b["counts"]))
            t_copy = SPR.timed_copy(c, b["copy"], b["labels"], h * w * 4)
            t = SR.timed(c, "centrelines", lambda: L.infur_centrelines_dev(c.h, b["labels"], 4, b["kind"], b["d2"], h, w, 1, NONE, max_links, b["records"], rows,
                                                                           b["vertices"], vrows, b["counts"]))
            counts = np.empty(8, np.uint32)
            c.check(L.infur_memcpy_d2h(c.h, counts.ctypes.data, b["counts"], 32))
            rec = np.empty((min(rows, int(counts[0])), 8), np.uint32)
            if rec.size:
                c.check(L.infur_memcpy_d2h(c.h, rec.ctypes.data, b["records"], rec.nbytes))
            longest = int((rec[:, 5] + rec[:, 6]).max()) if rec.size else 0
            print(row(name, h, w, int(n[0]), counts.tolist(), longest, max_links, t, t_skel, t_outl, t_copy), flush=True)
            for d in b.values():
                L.infur_dev_free(c.h, d)


def main(argv):
    if "--dry-run" in argv:
        return dry_run()
    measure(H, W_)


if __name__ == "__main__":
    main(sys.argv[1:])
