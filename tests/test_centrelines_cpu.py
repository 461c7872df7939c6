"""Centrelines without a GPU: tests/centrelines_ref.py on its own -- the header's worked example, every pixel in its branch, the link
sums against Skeleton's -- and the surface."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import centrelines_ref as CL  # noqa: E402
import regions_ref as R  # noqa: E402
import skeleton_ref as S  # noqa: E402

from infur_amd import _lib  # noqa: E402

PLANES = {"smooth270x480": functools.partial(R.smooth, 270, 480), "noise65x130": functools.partial(R.noise, 65, 130, 3),
          "plus130x130": functools.partial(S.plus, 130, 130), "checkerboard9x11": functools.partial(R.checkerboard, 9, 11),
          "single65x130": functools.partial(R.single, 65, 130), "smooth33x63": functools.partial(R.smooth, 33, 63)}


def test_the_worked_example_of_the_header():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    text = " ".join(header[header.index("EXAMPLE.  The plane of Skeleton's example"):header.index("No pruning of spurs (a record")].replace("*", " ").split())
    plane = np.array([[1, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 2], [0, 0, 0, 0, 0, 2, 0]], np.uint8)
    kind = S.skeleton(plane, None, 0, 0, 3)[0]
    rec, vert, counts = CL.centrelines(plane, kind, None, 0)
    assert "records (0, 4, 1, 8, 11, 3, 0, 0) and (4, 2, 2, 20, 26, 0, 1, 0), vertices 8 9 10 11 20 26, counts (2, 6, 4, 4, 4, 0, 1, 0)" in text
    assert rec.tolist() == [[0, 4, 1, 8, 11, 3, 0, 0], [4, 2, 2, 20, 26, 0, 1, 0]] and vert.tolist() == [8, 9, 10, 11, 20, 26]
    assert counts.tolist() == [2, 6, 4, 4, 4, 0, 1, 0]
    assert "records (0, 2, 1, 8, 11, 3, 0, 0) and (2, 2, 2, 20, 26, 0, 1, 0), vertices 8 11 20 26" in text
    rec, vert, counts = CL.centrelines(plane, kind, None, 0, corners=True)
    assert rec.tolist() == [[0, 2, 1, 8, 11, 3, 0, 0], [2, 2, 2, 20, 26, 0, 1, 0]] and vert.tolist() == [8, 11, 20, 26]
    assert counts.tolist() == [2, 4, 4, 4, 4, 0, 1, 0]


@pytest.mark.parametrize("name", sorted(PLANES))
def test_every_pixel_lies_in_its_branch_and_the_links_are_skeletons(name):
    plane = PLANES[name]()
    kind, _, sk = S.skeleton(plane)
    rec, vert, counts = CL.centrelines(plane, kind)
    kept, link = CL.links(plane, kind)
    path = (kept & (link.sum(0) == 2)).ravel()
    interior = np.concatenate([vert[o + 1:o + c - 1] for o, c in rec[:, :2]] + [np.zeros(0, np.uint32)])
    times = np.bincount(interior, minlength=plane.size) + np.bincount(rec[rec[:, CL.A] == rec[:, CL.B], CL.A], minlength=plane.size) * path
    assert (times[path] == 1).all() and not np.bincount(interior, minlength=plane.size)[~path].any()
    assert (np.bincount(vert, minlength=plane.size) > 0).tolist() == kept.ravel().tolist()
    assert rec[:, CL.ORTHO].sum() == sk[S.C_ORTHO] and rec[:, CL.DIAG].sum() == sk[S.C_DIAG] == counts[CL.C_DIAG]
    assert counts[CL.LINKS] == sk[S.C_ORTHO] + sk[S.C_DIAG] and (rec[:, CL.COUNT] == rec[:, CL.ORTHO] + rec[:, CL.DIAG] + 1).all()
    assert (np.diff(8 * rec[:, CL.A].astype(np.int64)) >= 0).all() and counts[CL.BRANCHES] == len(rec) and counts[CL.VERTICES] == len(vert)


def test_surface_and_the_rate_script_without_a_device():
    for s in ("infur_centrelines", "infur_centrelines_dev", "infur_frame_centrelines", "infur_frame_centrelines_dev"):
        assert s in _lib.SIGNATURES
    assert _lib.FEATURE_CENTRELINES == 32768 and _lib.load().infur_features() & _lib.FEATURE_CENTRELINES and _lib.ABI_VERSION == 7
    assert (CL.OFFSET, CL.B, CL.MIN_H, CL.WORDS, CL.RINGS, CL.STATUS, CL.CORNERS) == (
        _lib.CENTRELINE_OFFSET, _lib.CENTRELINE_B, _lib.CENTRELINE_MIN_H, _lib.CENTRELINE_WORDS, _lib.CENTRELINES_RINGS, _lib.CENTRELINES_STATUS,
        _lib.CENTRELINES_CORNERS)
    from infur_amd.processors import centreline_features
    feats = centreline_features(np.array([[0, 4, 7, 8, 8, 1, 2, 9]], np.uint32), np.array([8, 9, 17, 8], np.uint32), 7)
    assert feats == [{"value": 7, "vertices": [(1, 1), (2, 1), (3, 2), (1, 1)], "length": round(1 + 2 * 2 ** 0.5, 2), "narrowest": 6.0, "closed": True}]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "centrelines_rate.py"), "--dry-run"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and sum("27x48" in ln for ln in r.stdout.splitlines()) == 3, r.stdout + r.stderr
