"""The case table of tests/history.py, checked without a GPU: a later edit of a size, an index or the walk must not quietly turn
tests/test_gpu_history.py into a test of nothing -- a poison frame that is not larger, two frames that are the same frame, a walk
that gets its stale buffers trimmed away, a target whose tiles are all whole."""
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import history as H  # noqa: E402

from infur_amd import weights as W  # noqa: E402


def test_the_table_is_the_one_the_suite_documents():
    assert H.MODES == ["f32", "f32s", "f32x", "f16", "f16hl", "i8"]
    assert H.TARGETS == [(75, 109), (66, 130), (17, 33), (5, 7), (1, 1)]
    assert H.BIG == (136, 248) and H.FULL_TARGET in H.TARGETS
    src = open(os.path.join(H.ROOT, "infur_amd", "csrc", "infur_rt.h")).read()
    assert int(re.search(r"kPoolTrimAfter\s*=\s*(\d+)", src).group(1)) == H.POOL_TRIM_AFTER


@pytest.mark.parametrize("target", H.TARGETS)
def test_big_is_no_smaller_in_any_tensor(target):
    big, tgt = H.tensor_elems(H.BIG), H.tensor_elems(target)
    assert len(big) == len(tgt) == len(W.graph(50))
    assert all(b >= t for b, t in zip(big, tgt))
    assert all(b > t for b, t in zip(big, tgt))  # (and in fact larger in every one)
    assert H.BIG[0] * H.BIG[1] > target[0] * target[1]  # the frame itself: st_in, st_rgba


@pytest.mark.parametrize("target", H.TARGETS)
def test_near_is_larger_in_some_tensors_and_equal_in_others(target):
    """every NEAR frame is >= the target in every tensor and larger in at least one; the first is (h+2, w+2); at least one of them has
    tensors of exactly the target's size as well (from (5, 7) the first has none: history.near_sizes adds (h+2, w+1))"""
    tgt = H.tensor_elems(target)
    nears = H.near_sizes(target)
    assert nears[0] == (target[0] + 2, target[1] + 2) and 1 <= len(nears) <= 2
    some_equal = False
    for near in nears:
        n = H.tensor_elems(near)
        assert all(a >= b for a, b in zip(n, tgt)), near
        assert any(a > b for a, b in zip(n, tgt)), near
        some_equal = some_equal or any(a == b for a, b in zip(n, tgt))
    assert some_equal
    if target != (5, 7):
        assert len(nears) == 1  # (h+2, w+2) alone has both


def test_near_of_the_first_target_is_the_documented_one():
    """(75, 109) -> (77, 111): pooled stem 20x28 against 19x28, the same 10x14 from layer2 on"""
    def dims(size):
        return {spec.name: (oh, ow) for spec, _, _, oh, ow in W.plan(*size)}

    t, n = dims((75, 109)), dims((77, 111))
    assert t["backbone.layer1.0.conv1"] == (19, 28) and n["backbone.layer1.0.conv1"] == (20, 28)
    assert t["backbone.layer2.0.conv2"] == (10, 14) == n["backbone.layer2.0.conv2"]
    assert W.lowres_dims(75, 109) == (10, 14) == W.lowres_dims(77, 111)


@pytest.mark.parametrize("loud", [True, False])
@pytest.mark.parametrize("target", H.TARGETS)
def test_no_two_frames_of_a_walk_are_the_same_frame(target, loud):
    steps = H.walk_steps(target, loud=loud)
    poison = [(size, index) for what, size, index, _, _ in steps if what == "poison"]
    tgt = {(size, index) for what, size, index, _, _ in steps if what == "target"}
    assert tgt == {(target, H.target_index(target))}
    assert len(set(poison)) == len(poison) and not (set(poison) & tgt)
    # the four stages, in order: BIG, NEAR, SAME, BIG through the other model; a target after each
    kinds = [(what, size, which) for what, size, _, which, _ in steps]
    assert kinds[0] == ("poison", H.BIG, "normal") and kinds[-2] == ("poison", H.BIG, "loud" if loud else "normal")
    assert ("poison", target, "normal") in kinds
    assert all(kinds[i][0] == "target" and kinds[i][2] == "normal" for i in range(1, len(kinds), 2))
    assert all(kinds[i][0] == "poison" for i in range(0, len(kinds), 2))
    assert sum(1 for k in kinds if k[0] == "target") == 3 + len(H.near_sizes(target))


@pytest.mark.parametrize("target", H.TARGETS)
def test_no_walk_reaches_the_pool_trim(target):
    """the runtime trims the pool at the frame that kPoolTrimAfter frames of the same size precede: no walk has four equal
    consecutive sizes, the second forward of the full-resolution read-back counted"""
    sizes = H.forward_sizes(H.walk_steps(target))
    assert H.longest_equal_run(sizes) < H.POOL_TRIM_AFTER
    assert H.longest_equal_run([1, 1, 2, 2, 2, 1]) == 3  # (the helper itself)


def wino_sub_extent(n, d):
    """winograd.hip: geom() -- a dilation-d conv is d*d plain convs over the sub-grids; each covers ceil(n / d) rows or columns"""
    return (n + d - 1) // d


def wino_num_tiles(h, w, d, mt):
    """winograd.hip: wino_num_tiles, restated"""
    return d * d * ((wino_sub_extent(h, d) + mt - 1) // mt) * ((wino_sub_extent(w, d) + mt - 1) // mt)


def test_the_first_target_has_a_partial_tile_for_every_dilation_and_tile():
    """(75, 109): for each dilation 1, 2, 4 and each tile F(2x2), F(4x4), F(6x6), some stride-1 3x3 conv of that dilation has a
    sub-grid extent that is no multiple of the tile in at least one direction.  (The low-res map, 10x14, is even both ways: for
    dilation 1 and F(2x2) the partial tiles are layer1's, on the 19x28 pooled map.)"""
    by_dil = {}
    for spec, ih, iw, oh, ow in W.plan(75, 109):
        if spec.k == 3 and spec.stride == 1:
            assert (ih, iw) == (oh, ow)
            by_dil.setdefault(spec.dil, set()).add((ih, iw))
    assert sorted(by_dil) == [1, 2, 4]
    assert by_dil[2] == {(10, 14)} and by_dil[4] == {(10, 14)} and by_dil[1] == {(19, 28), (10, 14)}
    for d, maps in by_dil.items():
        for mt in (2, 4, 6):
            ragged = [(h, w) for h, w in maps if wino_sub_extent(h, d) % mt or wino_sub_extent(w, d) % mt]
            assert ragged, (d, mt)
            for h, w in ragged:  # the tiles cover more than the map: there IS an edge to get wrong
                assert wino_num_tiles(h, w, d, mt) * mt * mt > d * d * wino_sub_extent(h, d) * wino_sub_extent(w, d)
    # dilation 4 over 10 rows: sub-grids of 3, 3, 2, 2 rows -- the last tile row of two of them lies outside the map
    assert 10 % 4 != 0 and [len(range(r, 10, 4)) for r in range(4)] == [3, 3, 2, 2]
    # the low-res map is the dilated convs' and the heads': not a multiple of 4 or 6 in either direction
    assert all(n % mt for n in (10, 14) for mt in (4, 6))


def test_first_difference_names_key_index_and_values():
    import numpy as np

    a = {"lo": np.zeros((2, 3), np.float32), "rgba": np.zeros((2, 2, 4), np.uint8)}
    b = {k: v.copy() for k, v in a.items()}
    assert H.first_difference(a, b) is None
    b["rgba"][1, 0, 2] = 7
    msg = H.first_difference(a, b)
    assert msg.startswith("rgba: 1 of 16") and "(1, 0, 2)" in msg and "7" in msg
    b["lo"][0, 1] = np.float32("nan")  # bits, not values: a NaN differs from a number, -0.0 from 0.0
    assert "lo:" in H.first_difference(a, b) and "(0, 1)" in H.first_difference(a, b)
    c = {"lo": np.array([0.0], np.float32)}
    assert H.first_difference(c, {"lo": np.array([-0.0], np.float32)}) is not None
    nan = {"lo": np.array([np.nan], np.float32)}
    assert H.first_difference(nan, {"lo": nan["lo"].copy()}) is None  # the same NaN is the same bytes
    assert "missing" in H.first_difference(a, {"lo": a["lo"]})
