"""Redact without a GPU: the reference the GPU tests use (tests/redact_ref.py) on frames whose answer is written out, and the bindings."""
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redact_ref as D  # noqa: E402
import regions_ref as R  # noqa: E402


def bgr(blue):
    f = np.zeros((1, len(blue), 3), np.uint8)
    f[0, :, 0] = blue
    return f


def test_the_header_example():
    frame, plane, select = bgr([10, 20, 90, 40, 50, 61]), np.array([[1, 1, 0, 1, 1, 1]], np.uint8), [0, 1]
    blue = lambda *a, **kw: D.redact(frame, plane, select, *a, **kw)[0][0, :, 0].tolist()  # noqa: E731
    assert blue(D.PIXELATE, 2) == [15, 15, 90, 40, 56, 56]
    assert blue(D.BLUR, 1) == [15, 15, 90, 45, 50, 56]
    assert blue(D.BLUR, 1, passes=2) == [15, 15, 90, 48, 50, 53]
    assert blue(D.BLUR, 1, invert=True) == blue(D.PIXELATE, 2, invert=True) == [10, 20, 90, 40, 50, 61]
    assert blue(D.FILL, colour=7, invert=True) == [10, 20, 7, 40, 50, 61]
    out, counts = D.redact(frame, plane, select, D.BLUR, 1, passes=2)
    assert counts.tolist() == [5, 0, 2, 0, 0, 0, 0, 0] and not out[..., 1:].any()
    assert D.redact(frame, plane, [0], D.FILL, invert=True)[1].tolist() == [6, 5, 0, 0, 0, 0, 0, 0]  # value 1 lies beyond a one-row table
    assert D.redact(frame, plane, [0, 0], D.BLUR, 1)[1].tolist() == [0, 0, 1, 0, 0, 0, 0, D.NOTHING]


@pytest.mark.parametrize("mode,size", [(D.PIXELATE, 2), (D.BLUR, 1)])
def test_a_tie_rounds_up_and_a_constant_colour_stays(mode, size):
    assert D.redact(bgr([0, 1]), np.ones((1, 2), np.uint8), [0, 1], mode, size)[0][0, :, 0].tolist() == [1, 1]
    plane = R.smooth(40, 70, seed=2)
    value = int(plane[20, 35])
    frame = np.random.default_rng(1).integers(0, 256, (40, 70, 3), dtype=np.uint8)
    frame[plane == value] = [3, 250, 77]
    out, _ = D.redact(frame, plane, np.arange(256) == value, mode, size * 3, passes=3)
    assert (out == frame).all()


@pytest.mark.parametrize("mode,size", [(D.PIXELATE, 5), (D.BLUR, 3)])
@pytest.mark.parametrize("invert", [False, True])
def test_unselected_pixels_do_not_contribute(mode, size, invert):
    plane, rng = R.noise(23, 31, 3, seed=4), np.random.default_rng(5)
    frame = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    out, _ = D.redact(frame, plane, [0, 1], mode, size, invert=invert)
    sel, _ = D.selection(plane, [0, 1], invert)
    other = frame.copy()
    other[~sel] = rng.integers(0, 256, (int((~sel).sum()), 3), dtype=np.uint8)
    again, _ = D.redact(other, plane, [0, 1], mode, size, invert=invert)
    assert (again[sel] == out[sel]).all() and (again[~sel] == other[~sel]).all() and (out[~sel] == frame[~sel]).all()


def test_the_four_calls_are_bound():
    names = ("infur_redact", "infur_redact_dev", "infur_frame_redact", "infur_frame_redact_dev")
    assert all(name in _lib.SIGNATURES for name in names)  # (fails on the code without Redact)
    assert len(_lib.SIGNATURES["infur_redact"][1]) == 15 and len(_lib.SIGNATURES["infur_frame_redact"][1]) == 23
    assert _lib.FEATURE_REDACT == 131072 and (D.FILL, D.PIXELATE, D.BLUR) == (_lib.REDACT_FILL, _lib.REDACT_PIXELATE, _lib.REDACT_BLUR)
    assert (D.C_SELECTED, D.C_OUTSIDE, D.C_PASSES, D.C_STATUS) == (0, 1, 2, 7) == (_lib.REDACT_COUNT_SELECTED, _lib.REDACT_COUNT_OUTSIDE, _lib.REDACT_COUNT_PASSES, _lib.REDACT_COUNT_STATUS)
