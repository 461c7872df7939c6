"""Skeleton without a GPU: tests/skeleton_ref.py on its own -- topology, idempotence, the header's worked example -- and the surface."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import regions_ref as R  # noqa: E402
import skeleton_ref as S  # noqa: E402

from infur_amd import _lib  # noqa: E402

PLANES = {"single": R.single(20, 31), "smooth": R.smooth(33, 63, 5, 4, 8), "noise": R.noise(24, 40, 3), "serpentine": R.serpentine(21, 30),
          "spiral": R.spiral(25, 25), "staircase": R.staircase(20, 30), "checkerboard": R.checkerboard(9, 11), "line": np.ones((1, 70), np.uint8),
          "bar": np.ones((2, 70), np.uint8), "plus": S.plus(40, 40)}


def components(mask_plane, keep):
    """the number of 8-connected components per value among the pixels of `keep`"""
    labels, _, n = R.label(np.where(keep, mask_plane.astype(np.uint32) + 1, 0).astype(np.uint8), connectivity=8, flags=_lib.REGIONS_SKIP_BACKGROUND)
    return n


@pytest.mark.parametrize("name", sorted(PLANES))
def test_components_are_kept_and_nothing_is_left_to_remove(name):
    plane = PLANES[name]
    kind, table, counts = S.skeleton(plane)
    alive = kind > 0
    assert components(plane, alive) == components(plane, np.ones(plane.shape, bool))
    assert not counts[S.STATUS] and counts[S.ROUNDS] <= min(plane.shape) - 1 + (min(plane.shape) == 1)
    assert counts[S.KEPT] + counts[S.REMOVED] == plane.size and table[:, S.PIXELS].sum() == counts[S.KEPT] == alive.sum()
    assert not S.dies(plane, alive, 1).any() and not S.dies(plane, alive, 2).any()  # a second pair of sub-iterations removes nothing
    assert table[:, S.ORTHO].sum() == counts[S.C_ORTHO] and table[:, S.ENDS].sum() == (kind == 2).sum() == counts[S.C_ENDS]
    cut = S.skeleton(plane, max_rounds=1)[2]
    assert cut[S.ROUNDS] <= 1 and cut[S.STATUS] == S.UNFINISHED


def test_a_square_keeps_one_pixel_and_a_line_stays():
    assert S.skeleton(np.ones((2, 2), np.uint8))[2].tolist() == [1, 3, 1, 0, 0, 0, 0, 0]
    kind, table, counts = S.skeleton(PLANES["line"], height=np.arange(70, dtype=np.uint32).reshape(1, 70) + 5)
    assert (kind[0, 1:-1] == 3).all() and table[1].tolist() == [70, 2, 0, 69, 0, 0, 5, 74] and counts[S.ROUNDS] == 0


def test_the_worked_example_of_the_header():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    text = " ".join(header[header.index("EXAMPLE.  h = 4, w = 7"):header.index("WHAT IT DOES NOT DO.  No pruning")].replace("*", " ").split())
    plane = np.array([[1, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 2], [0, 0, 0, 0, 0, 2, 0]], np.uint8)
    kind, table, counts = S.skeleton(plane, None, 0, 0, 3)
    assert "(0, 0, 0, 0, 0, NONE, 0, 0), (4, 2, 0, 3, 0, 8, 0, 0), (2, 2, 0, 0, 1, 20, 0, 0) and the counts are (6, 14, 2, 4, 0, 3, 1, 0)" in text
    assert kind.tolist() == [[0] * 7, [0, 2, 3, 3, 2, 0, 0], [0, 0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 2, 0]]
    assert table.tolist() == [[0, 0, 0, 0, 0, S.NONE, 0, 0], [4, 2, 0, 3, 0, 8, 0, 0], [2, 2, 0, 0, 1, 20, 0, 0]] and counts.tolist() == [6, 14, 2, 4, 0, 3, 1, 0]
    assert "max_rounds = 2 gives the same result with STATUS = 1" in text and "counts (12, 8, 1, 2, 10, 13, 1, 1)" in text
    two, one = S.skeleton(plane, None, 0, 2, 3), S.skeleton(plane, None, 0, 1, 3)
    assert (two[0] == kind).all() and two[2].tolist() == [6, 14, 2, 4, 0, 3, 1, 1] and one[2].tolist() == [12, 8, 1, 2, 10, 13, 1, 1]
    assert one[0].tolist() == [[0, 4, 6, 6, 6, 4, 0], [0, 4, 6, 6, 6, 4, 0], [0, 0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 2, 0]]


def test_surface_and_the_rate_script_without_a_device():
    for s in ("infur_skeleton", "infur_skeleton_dev", "infur_frame_skeleton", "infur_frame_skeleton_dev"):
        assert s in _lib.SIGNATURES
    assert _lib.FEATURE_SKELETON == 16384 and _lib.load().infur_features() & _lib.FEATURE_SKELETON and _lib.ABI_VERSION == 7
    assert (S.PIXELS, S.FIRST, S.MAX_H, S.WORDS, S.ROUNDS, S.STATUS) == (_lib.SKELETON_PIXELS, _lib.SKELETON_FIRST, _lib.SKELETON_MAX_H, _lib.SKELETON_WORDS,
                                                                        _lib.SKELETON_ROUNDS, _lib.SKELETON_STATUS)
    from infur_amd.processors import skeleton_summary
    recs = skeleton_summary(np.array([[0, 0, 0, 0, 0, S.NONE, 0, 0], [4, 2, 0, 3, 1, 8, 4, 9]], np.uint32), np.array([4, 14, 2, 2, 0, 3, 1, 0], np.uint32))
    assert recs[0]["rounds"] == 2 and not recs[0]["unfinished"] and len(recs) == 2
    assert recs[1] == {"value": 1, "pixels": 4, "length": 4.41, "ends": 2, "junctions": 0, "first": 8, "narrowest": 4.0, "widest": 6.0}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "skeleton_rate.py"), "--dry-run"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and sum("27x48" in ln for ln in r.stdout.splitlines()) == 3, r.stdout + r.stderr
