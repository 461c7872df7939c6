"""Split without a GPU: tests/split_ref.py against a prototype's numbers, the header's worked example, identities, the surface."""
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
import split_ref as S  # noqa: E402

from infur_amd import _lib  # noqa: E402

NONE = 0xFFFFFFFF


def sizes_of(plane, core, value=1):
    labels, table, counts = S.split(plane, S.dist2(plane), core)
    return sorted(int(t[S.PIXELS]) for t in table if t[S.VALUE] == value), counts


@pytest.mark.parametrize("core,sizes", [(4, [672]), (16, [321, 351]), (36, [321, 351]), (64, [321, 351]), (200, [672])])
def test_the_dumbbell_splits_at_its_neck(core, sizes):
    got, counts = sizes_of(S.dumbbell(25, 52, r=10, neck=2), core)
    assert got == sizes and (counts[S.BASINS], counts[S.PAIRS]) == (22, 21)


@pytest.mark.parametrize("plane,basins,pairs", [(S.bar(), 9, 8), (S.band(24, 50), 37, 34)])
def test_a_bar_and_a_diagonal_band_stay_whole(plane, basins, pairs):
    for core in (0, 1, 4, 9, 16, 36, 64, 200, NONE):
        got, counts = sizes_of(plane, core)
        assert got == [int((plane == 1).sum())] and (counts[S.BASINS], counts[S.PAIRS]) == (basins, pairs)


def test_the_worked_example_of_the_header():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    text = " ".join(header[header.index("EXAMPLE.  h = 1, w = 9"):header.index("WHAT IT DOES NOT DO.  No 8-neighbour")].replace("*", " ").split())
    plane, height = np.ones((1, 9), np.uint8), np.array([[1, 4, 9, 4, 1, 4, 9, 4, 1]], np.uint32)
    assert "height = 1 4 9 4 1 4 9 4 1" in text and "SADDLE = min(1, 4) = 1 and FIRST = 8" in text
    labels, table, counts = S.split(plane, height, 4)
    assert "labels 0 0 0 0 0 1 1 1 1, rows (1, 5, 0, 2, 9, 1) and (1, 4, 5, 6, 9, 1), counts (2, 2, 1, 1, 2, 1, 0, 0)" in text
    assert labels.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1, 1]] and table.tolist() == [[1, 5, 0, 2, 9, 1], [1, 4, 5, 6, 9, 1]]
    assert counts.tolist() == [2, 2, 1, 1, 2, 1, 0, 0]
    assert "row (1, 9, 0, 2, 9, 0), counts (1, 2, 1, 1, 2, 0, 0, 0)" in text and "the same row, counts (1, 2, 1, 1, 0, 0, 1, 0)" in text
    for core, want in ((1, [1, 2, 1, 1, 2, 0, 0, 0]), (10, [1, 2, 1, 1, 0, 0, 0, 0])):  # (ROUNDS, 1 in the header, is the device's word)
        labels, table, counts = S.split(plane, height, core)
        assert not labels.any() and table.tolist() == [[1, 9, 0, 2, 9, 0]] and counts.tolist() == want


@pytest.mark.parametrize("skip", (None, 0))
def test_identities_and_the_two_ends_of_core(skip):
    plane = R.smooth(33, 63, 4, 3, 8)
    height = S.dist2(plane, skip)
    kept = plane != skip if skip is not None else np.ones(plane.shape, bool)
    for core in (0, 4, 16, NONE):
        labels, table, counts = S.split(plane, height, core, skip)
        assert table[:, S.PIXELS].sum() == kept.sum() and counts[S.SEGMENTS] >= len(np.unique(plane[kept]))
        assert ((labels == NONE) == ~kept).all()
        for i, row in enumerate(table):  # every segment lies inside one value, and its rows say where
            assert (plane[labels == i] == row[S.VALUE]).all() and labels.ravel()[row[S.FIRST]] == i == labels.ravel()[row[S.PEAK]]
            assert height.ravel()[row[S.PEAK]] == row[S.HEIGHT] == height[labels == i].max()
        if core in (0, NONE):  # exactly Regions' 4-connected components, in Regions' numbering
            ref, _, n = R.label(plane, connectivity=4, min_pixels=0)
            if skip is None:
                assert n == counts[S.SEGMENTS] and (labels == ref).all() and not table[:, S.NECK].any()
            else:
                comps = sorted({int(v) for v in ref[kept]})
                assert len(comps) == counts[S.SEGMENTS] and (np.searchsorted(comps, ref[kept]) == labels[kept]).all()


def test_surface_and_the_rate_script_without_a_device():
    for s in ("infur_split", "infur_split_dev", "infur_frame_split", "infur_frame_split_dev"):
        assert s in _lib.SIGNATURES
    assert _lib.FEATURE_SPLIT == 8192 and _lib.load().infur_features() & _lib.FEATURE_SPLIT and _lib.ABI_VERSION == 7
    assert (S.PIXELS, S.NECK, S.WORDS, S.SPLIT_VALUES, S.STATUS) == (_lib.SPLIT_PIXELS, _lib.SPLIT_NECK, _lib.SPLIT_WORDS, _lib.SPLIT_SPLIT_VALUES,
                                                                     _lib.SPLIT_STATUS)
    assert "pub struct HipSplit" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    from infur_amd.processors import split_core, split_summary
    assert [split_core(px) for px in (0, 1, 2, 7, 8, 24)] == [0, 1, 1, 16, 16, 144] and split_summary(np.arange(8))["split_values"] == 5
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "split_rate.py"), "--dry-run"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("| ")]
    assert r.returncode == 0 and sum("27x48" in ln for ln in rows) == 6 and sum("advance_split" in ln for ln in rows) == 1, r.stdout + r.stderr
