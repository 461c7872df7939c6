"""Expand (every open pixel takes the value of its exact nearest seed) without a GPU: the reference the GPU tests use
(tests/expand_ref.py) on hand-made planes whose answer is written out, and against scipy's exact transform where scipy imports."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import expand_ref as E  # noqa: E402
import regions_ref as R  # noqa: E402

N = E.NONE


def test_the_header_example():
    out, dist2, source, table, counts = E.expand(np.array([[0, 0, 5, 0, 0, 0, 7]], np.uint8), 0, reach=1, rows=8)
    assert source.tolist() == [[2, 2, 2, 2, 2, 6, 6]] and dist2.tolist() == [[4, 1, 0, 1, 4, 1, 0]] and out.tolist() == [[0, 5, 5, 5, 0, 7, 7]]
    assert table[5].tolist() == [1, 2, 1, 1] and table[7].tolist() == [1, 1, 1, 5]
    assert all(table[v].tolist() == [0, 0, 0, N] for v in (0, 1, 2, 3, 4, 6))
    assert counts.tolist() == [2, 5, 3, 2, 4, 0, 0, 0]


@pytest.mark.parametrize("plane,at,source", [
    ([[3, 0, 4]], (0, 1), 0),                       # equidistant horizontally: the smaller x
    ([[3], [0], [4]], (1, 0), 0),                   # vertically: the smaller y
    ([[0, 0, 4], [0, 0, 0], [3, 0, 0]], (1, 1), 2),  # diagonally: the smaller y, although its x is larger
    ([[3, 0, 0], [0, 0, 0], [0, 0, 4]], (1, 1), 0),
    ([[0, 3, 0], [4, 0, 5], [0, 6, 0]], (1, 1), 1),  # four at distance 1: the first in raster order
])
def test_ties_go_to_the_smallest_index(plane, at, source):
    plane = np.array(plane, np.uint32)
    out, _, src, _, _ = E.expand(plane, 0)
    assert src[at] == source and out[at] == plane.ravel()[source]


def test_reach_squared_hit_exactly_and_no_seed():
    p = np.zeros((5, 6), np.uint8)
    p[0, 0] = 9
    out, dist2, _, table, counts = E.expand(p, 0, reach=5, rows=10)
    assert dist2[3, 4] == 25 == dist2[4, 3] and out[3, 4] == 9 == out[4, 3] and out[4, 4] == 0 and dist2[4, 4] == 32  # 25 <= 5^2 < 32
    assert table[9].tolist() == [1, int((dist2 <= 25).sum()) - 1, 25, 5] and counts[E.C_MAX_D2] == 41
    assert (E.expand(p, 0, reach=4)[0] != 0).sum() == (dist2 <= 16).sum()
    out, dist2, source, table, counts = E.expand(np.zeros((2, 3), np.uint8), 0, rows=1)
    assert (out == 0).all() and (dist2 == N).all() and (source == N).all() and table.tolist() == [[0, 0, 0, N]]
    assert counts.tolist() == [0, 6, 0, 6, 0, 0, 0, E.NO_SEED]
    out, dist2, source, _, counts = E.expand(np.full((2, 3), 7, np.uint8), 0)  # all seeds
    assert (out == 7).all() and (dist2 == 0).all() and source.ravel().tolist() == list(range(6)) and counts.tolist() == [6, 0, 0, 0, 0, 0, 0, 0]
    assert E.expand(np.zeros((0, 4), np.uint8), 0, rows=2)[3].tolist() == [[0, 0, 0, N]] * 2


def test_dist2_equals_scipys_exact_transform():
    ndimage = pytest.importorskip("scipy.ndimage")
    for k in (R.smooth(40, 70, seed=1), R.noise(33, 63, 3, seed=2), R.checkerboard(7, 65)):
        d = ndimage.distance_transform_edt(k == k[0, 0])
        assert (E.expand(k, int(k[0, 0]))[1] == np.rint(d * d)).all()
