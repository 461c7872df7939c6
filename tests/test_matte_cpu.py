"""Matte and Composite without a GPU: the reference the GPU tests use (tests/matte_ref.py) on the header's written-out example, the
weight rows the formula gives, and the bindings."""
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matte_ref as M  # noqa: E402


def test_the_header_example():
    frame = np.zeros((1, 6, 3), np.uint8)
    frame[0, :, 0] = [10, 10, 10, 200, 200, 200]
    plane, select = np.array([[1, 1, 1, 1, 0, 0]], np.uint8), [0, 1]
    alpha, counts = M.matte(frame, plane, select, 1, 12)
    assert alpha.tolist() == [[255, 255, 255, 128, 85, 0]] and counts.tolist() == [4, 0, 1, 2, 3, 0, 0, 0]
    assert M.matte(frame, plane, select, 2, 12)[0].tolist() == [[255, 255, 255, 85, 85, 85]]
    assert M.matte(frame, plane, select, 1, 12, M.INVERT)[0].tolist() == [[0, 0, 0, 127, 170, 255]]
    assert M.matte(frame, plane, select, 1, 12, M.CONF, conf=np.array([[200, 200, 200, 200, 7, 7]], np.uint8))[0].tolist() == [[200, 200, 200, 100, 67, 0]]
    alpha, counts = M.matte(frame, plane, [0], 1, 12)  # value 1 lies beyond a one-row table
    assert not alpha.any() and counts.tolist() == [0, 4, 6, 0, 0, 0, 0, M.NOTHING]
    steps = np.array([[0, 1, 127, 128, 254, 255]], np.uint8)
    assert M.composite(frame, steps, M.COLOUR, colour=255)[0, :, 0].tolist() == [255, 254, 133, 227, 200, 200]
    assert M.composite(frame, steps, M.IMAGE, back=255 - frame)[0, :, 1].tolist() == [255, 254, 128, 127, 1, 0]
    assert M.composite(frame, steps, M.CUTOUT)[0, 3].tolist() == [200, 0, 0, 128]


@pytest.mark.parametrize("sigma,d,want", [(1, (0, 1, 2, 3), (4096, 2048, 819, 409)), (12, (0, 12, 24, 100, 765), (4096, 2048, 819, 58, 1)),
                                          (255, (0, 255, 765), (4096, 2048, 409))])
def test_the_weights_the_formula_gives(sigma, d, want):
    assert tuple(int(M.weights(sigma)[k]) for k in d) == want


def test_a_uniform_window_keeps_its_value():
    frame = np.random.default_rng(2).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    conf = np.full((9, 11), 77, np.uint8)
    assert (M.matte(frame, np.ones((9, 11), np.uint8), [0, 1], 3, 5, M.CONF, conf)[0] == 77).all()
    assert (M.matte(frame, np.ones((9, 11), np.uint8), [0, 1], 3, 5)[0] == 255).all()


def test_the_six_calls_are_bound():
    arity = {"infur_matte": 14, "infur_matte_dev": 14, "infur_composite": 9, "infur_composite_dev": 9, "infur_frame_matte": 25, "infur_frame_matte_dev": 25}
    assert all(name in _lib.SIGNATURES for name in arity)  # (fails on the code without Matte)
    assert {name: len(_lib.SIGNATURES[name][1]) for name in arity} == arity
    assert _lib.FEATURE_MATTE == 524288 and (M.INVERT, M.CONF, M.NOTHING) == (_lib.MATTE_INVERT, _lib.MATTE_CONF, _lib.MATTE_NOTHING)
    assert (M.COLOUR, M.IMAGE, M.CUTOUT) == (_lib.COMPOSITE_COLOUR, _lib.COMPOSITE_IMAGE, _lib.COMPOSITE_CUTOUT)
    assert (M.C_SELECTED, M.C_OUTSIDE, M.C_CLEAR, M.C_SOFT, M.C_OPAQUE, M.C_STATUS) == (0, 1, 2, 3, 4, 7) == (
        _lib.MATTE_COUNT_SELECTED, _lib.MATTE_COUNT_OUTSIDE, _lib.MATTE_COUNT_CLEAR, _lib.MATTE_COUNT_SOFT, _lib.MATTE_COUNT_OPAQUE, _lib.MATTE_COUNT_STATUS)
