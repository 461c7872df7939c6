"""Appearance without a GPU: the reference the GPU tests use (tests/appearance_ref.py) on the header's example, and the bindings."""
import os
import sys

import numpy as np

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import appearance_ref as A  # noqa: E402


def test_the_header_example():
    frame = np.zeros((1, 6, 3), np.uint8)
    frame[0, :, 0] = [10, 20, 90, 40, 50, 61]
    plane = np.array([[1, 1, 0, 1, 1, 1]], np.uint8)
    row0, row1 = [1, 90, 0, 0, 8100, 0, 0, 0, 0, 0, 1, 1], [5, 181, 0, 0, 8321, 0, 0, 0, 0, 0, 0, 5]
    table, hist, counts = A.appearance(frame, plane, 2)
    assert table.tolist() == [row0, row1] and counts.tolist() == [6, 0, 0, 2, 0, 0, 0, 0]
    assert hist[0, 1] == 1 and hist[1, 0] == 5 and hist.sum() == 6
    table, hist, counts = A.appearance(frame, plane, 2, A.SKIP, 0)
    assert table.tolist() == [[0] * 12, row1] and not hist[0].any() and counts.tolist() == [5, 1, 0, 1, 0, 0, 0, 0]
    table, hist, counts = A.appearance(frame, plane, 1)
    assert table.tolist() == [row0] and counts.tolist() == [1, 0, 5, 1, 0, 0, 0, 0]
    assert A.appearance(frame, plane, 2, A.SKIP, 0)[2][A.C_STATUS] == 0 and A.appearance(frame, plane * 0, 2, A.SKIP, 0)[2][A.C_STATUS] == A.NOTHING


def test_the_four_calls_are_bound():
    names = ("infur_appearance", "infur_appearance_dev", "infur_frame_appearance", "infur_frame_appearance_dev")
    assert all(name in _lib.SIGNATURES for name in names)  # (fails on the code without Appearance)
    assert [len(_lib.SIGNATURES[name][1]) for name in names] == [12, 12, 25, 25]
    assert _lib.FEATURE_APPEARANCE == 262144 and _lib.ABI_VERSION == 7
    older = ("SEGMENTS", "REGIONS", "TRACKS", "RUNS", "OUTLINES", "SIMPLIFY", "COVERAGE", "TRACK_MEMORY", "ANCHORS", "COMPARE", "SIEVE", "SHAPES",
             "RASTER", "SPLIT", "SKELETON", "CENTRELINES", "EXPAND", "REDACT")
    assert sorted(getattr(_lib, "FEATURE_" + name) for name in older) == [1 << k for k in range(18)]
    assert (A.SKIP, A.WORDS, A.BINS, A.NOTHING) == (_lib.APPEARANCE_SKIP, _lib.APPEARANCE_WORDS, _lib.APPEARANCE_BINS, _lib.APPEARANCE_NOTHING)
    assert (A.C_COUNTED, A.C_SKIPPED, A.C_OUTSIDE, A.C_VALUES, A.C_STATUS) == (
        _lib.APPEARANCE_COUNT_COUNTED, _lib.APPEARANCE_COUNT_SKIPPED, _lib.APPEARANCE_COUNT_OUTSIDE, _lib.APPEARANCE_COUNT_VALUES, _lib.APPEARANCE_COUNT_STATUS)
