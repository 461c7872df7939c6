"""The frame sizes of tests/forms.py, proved on the CPU: tests/edge_cover.py names the edge classes a frame puts a kernel into (GEMM
tail rows per BM, 3x3 taps against the border per dilation, Winograd phase lengths per tile, halo patch and tiling, workgroups of the
activation-in-register forms, stem / pool parities, decode widths), searches every frame of a 272 x 272 box for the classes it
reaches, and covers what forms.SIZES, NATURAL_SIZES and GEOM_SIZES miss with COVER_SIZES.  Here:

  * the four lists together reach EVERY class the box reaches -- no share is left out: the box bounds what is reachable;
  * COVER_SIZES is what the deterministic greedy search returns today, within both caps (16 sizes, none above 272 x 272);
  * the classes the old sizes alone miss are printed by family; they hold the M = 1 and M = BM - 1 (mod BM) tails of all three BM at
    every conv kind;
  * every class function is held against a brute-force restatement on tiny maps: taps counted by enumeration, tiles and phases
    counted by walking them, the halo plan's tiling by enumerating its candidates' costs.
"""
import itertools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import edge_cover as E  # noqa: E402
import forms as F  # noqa: E402

from infur_amd import weights as W  # noqa: E402

SPECS = W.graph(50)


def spec_named(name):
    return next(s for s in SPECS if s.name == name)


# ---- the cover ------------------------------------------------------------------------------------------------------------------------
def test_all_sizes_together_reach_every_class_of_the_box():
    universe, _ = E.reachable()
    have = E.classes_of(E.OLD_SIZES + E.COVER_SIZES)
    left = universe - have
    print(f"{len(universe)} classes reachable with 1 <= h, w <= {E.BOX}; SIZES reaches {len(E.classes_of(F.SIZES) & universe)}, "
          f"SIZES + NATURAL_SIZES + GEOM_SIZES {len(E.classes_of(E.OLD_SIZES) & universe)}, with COVER_SIZES {len(have & universe)}")
    assert not left, f"classes no committed size reaches: {sorted(left)}"
    assert len(universe) >= 250
    for fam in E.FAMILIES:  # every family has classes
        assert E.by_family(universe)[fam], fam


def test_cover_sizes_are_what_the_search_returns_and_respect_the_caps():
    cover = E.greedy_cover()
    print("greedy cover:", cover)
    assert cover == E.COVER_SIZES
    assert E.greedy_cover() == cover  # deterministic
    assert 0 < len(E.COVER_SIZES) <= E.MAX_SIZES == 16 and E.BOX == 272
    assert all(1 <= h <= E.BOX and 1 <= w <= E.BOX for h, w in E.COVER_SIZES)
    assert F.SIZE_SETS["cover"] is E.COVER_SIZES or F.SIZE_SETS["cover"] == E.COVER_SIZES
    assert all(F.PRE_FRAME[s] not in (s, None) for s in E.COVER_SIZES)
    # every size is there for something: each adds classes to all sizes before it
    have = set(E.classes_of(E.OLD_SIZES))
    for s in E.COVER_SIZES:
        new = E.frame_classes(*s) - have
        print(f"  {F.tag(s)}: {len(new)} new classes: {' '.join(sorted(new))}")
        assert new, s
        have |= new


def test_what_the_old_sizes_miss():
    universe, _ = E.reachable()
    missed = E.missed_by(E.OLD_SIZES)
    print(f"SIZES + NATURAL_SIZES + GEOM_SIZES miss {len(missed)} of {len(universe)} classes:")
    for fam, classes in E.by_family(missed).items():
        print(f"  {fam} ({len(classes)}): {' '.join(classes)}")
    assert missed
    for kind in ("1x1s1", "1x1s2", "3x3"):
        for bm in E.BMS:
            assert f"A/{kind}/bm{bm}/1" in missed and f"A/{kind}/bm{bm}/bm-1" in missed, (kind, bm)
    # ... and the issue's other examples: d < dim <= 2d at dilation 2, halo maps of 2-7, phase lengths of 0 (mod 6)
    assert {"B/d2/h/le_2d", "B/d2/w/le_2d", "X/halo8/h/2-7", "C/d1/h/mt6/0", "C/d4/w/mt6/0"} <= missed
    assert missed <= E.classes_of(E.COVER_SIZES)


def test_the_plan_separates_by_axis():
    """frame_classes walks one chain per axis and one set per distinct layer signature: the same classes as weights.plan layer by
    layer, on every committed size and a diagonal of the box"""
    sizes = E.OLD_SIZES + E.COVER_SIZES + [(n, 273 - n) for n in range(1, 273, 7)]
    for h, w in sizes:
        plan = W.plan(h, w)
        want = set()
        for spec, ih, iw, oh, ow in plan:
            want |= E.layer_classes(spec, ih, iw, oh, ow)
        want |= E.stem_classes(h, w, plan[0][3], plan[0][4]) | E.decode_classes(w, plan[-1][3], plan[-1][4])
        assert plan[-1][3:] == W.lowres_dims(h, w)
        assert E.frame_classes(h, w) == want, (h, w)


# ---- the class functions against brute force --------------------------------------------------------------------------------------------
def test_tail_case_by_walking_the_tiles():
    for bm in (32, 64, 128, 256):
        for m in range(1, 3 * bm + 3):
            tiles = [min(bm, m - m0) for m0 in range(0, m, bm)]  # rows of each tile
            if len(tiles) == 1 and tiles[0] < bm:
                want = "lt"
            elif tiles[-1] == bm:
                want = "0"
            else:
                want = {1: "1", bm - 1: "bm-1"}.get(tiles[-1], "other")
            assert E.tail_case(m, bm) == want, (m, bm)


def lost_taps(dim, d):
    """per output position of a pad = d, dilation d, stride 1 3x3 conv: how many of its three taps along one axis fall outside"""
    return [sum(1 for k in (-1, 0, 1) if not 0 <= x + k * d < dim) for x in range(dim)]


def test_border_case_by_counting_out_of_range_taps():
    for d in E.DILS:
        for dim in range(1, 4 * d + 4):
            lost = lost_taps(dim, d)
            want = "le_d" if set(lost) == {2} else "le_2d" if min(lost) >= 1 else "gt_2d"
            assert E.border_case(dim, d) == want, (dim, d, lost)
    s2 = spec_named("backbone.layer2.0.conv2")
    assert s2.stride == 2 and s2.dil == 1
    assert E.border_classes(s2, 5, 8) == {"B/s2/h/odd", "B/s2/w/even", "B/s2/h/gt_2d", "B/s2/w/gt_2d"}
    for n in range(1, 12):  # even input: the last output's right tap is inside; odd: it is the padding
        outs = W.conv_out(n, 3, 2, 1, 1)
        right = 2 * (outs - 1) - 1 + 2  # input index of the last output's right tap
        assert (right < n) == (n % 2 == 0), n
    d4 = spec_named("backbone.layer4.1.conv2")
    assert d4.dil == 4 and E.border_classes(d4, 4, 9) == {"B/d4/h/le_d", "B/d4/w/gt_2d"}


def test_phase_case_by_walking_the_phases():
    for d in E.DILS:
        for dim in range(1, 8 * d + 8):
            lengths = [len([x for x in range(dim) if x % d == p]) for p in range(d)]
            assert E.phase_lengths(dim, d) == lengths, (dim, d)
            for mt in E.TILES:
                n_tiles = -(-(-(-dim // d)) // mt)  # wino_num_tiles: every phase gets the tiles of the longest
                for ln in lengths:
                    used = [min(mt, ln - t * mt) for t in range(n_tiles) if ln - t * mt > 0]  # positions in each tile that holds any
                    if not used:
                        want = "empty"
                    elif ln < mt:
                        want = "lt"
                    elif used[-1] == mt:
                        want = "0"
                    else:
                        want = {mt - 1: "mt-1", 1: "1"}.get(used[-1], "other")  # (mt = 2: one position is both)
                    assert E.phase_case(ln, mt) == want, (dim, d, mt, ln)
    s = spec_named("backbone.layer4.1.conv2")
    assert E.wino_classes(s, 3, 13, 6) == {"C/d4/h/mt6/lt", "C/d4/h/mt6/empty", "C/d4/w/mt6/lt"}
    assert E.wino_classes(spec_named("backbone.layer2.1.conv2"), 19, 27, 6) == {"C/d1/h/mt6/1", "C/d1/w/mt6/other"}


def test_halo_axis_cases_by_walking_the_tiles():
    for dim in range(1, 70):
        tiles16 = [min(16, dim - t) for t in range(0, dim, 16)]
        if dim < 16:
            assert E.halo_axis_case(dim) == "lt16" and tiles16 == [dim]
            rows8 = [min(8, dim - t) for t in range(0, dim, 8)]
            want = "1" if dim == 1 else "2-7" if rows8 == [dim] and dim < 8 else "8" if rows8 == [8] else "9-15"
            assert E.halo8_case(dim) == want, dim
        else:
            last = tiles16[-1] % 16
            assert E.halo_axis_case(dim) == (str(last) if last in (0, 1, 8, 9, 15) else "other"), dim
            assert E.halo8_case(dim) == ("strip" if 1 <= tiles16[-1] <= 8 else "nostrip"), dim


def brute_tiling(oh, ow, d, cin, cout, bn, es):
    """halo_plan's choice by listing (cost, order) of every feasible (candidate, patch images) pair and taking the minimum"""
    cd = lambda a, b: -(-a // b)  # noqa: E731
    geoms = [("16x16", [(16, 16)], cd(oh, 16) * cd(ow, 16)), ("8x32", [(8, 32)], cd(oh, 8) * cd(ow, 32))]
    if oh >= 16 and 1 <= oh % 16 <= 8:
        geoms.append(("mixed", [(16, 16), (oh % 16, 32)], (oh // 16) * cd(ow, 16) + cd(ow, 32)))
    kchunks = cin * es // 128
    rows = []
    for order, (word, tiles, mtiles) in enumerate(geoms):
        for na in ([1] if kchunks == 1 or bn == 64 else [2, 1]):
            pieces = max(cd((th + 2 * d) * (tw + 2 * d), 8) for th, tw in tiles)
            lds = max(max(na * cd((th + 2 * d) * (tw + 2 * d), 8) * 1024 + 3 * bn * (128 if bn <= 128 else 64), 8 * 32 * 272) for th, tw in tiles)
            if lds > 160 * 1024 or pieces > 72:
                continue
            per_cu = 2 if bn <= 128 and na == 1 and lds <= 80 * 1024 else 1
            rounds = cd(mtiles * (cout // bn), 256 * per_cu) * (11 if na == 1 and kchunks > 1 else 10)
            rows.append(((rounds, mtiles, (tiles[0][0] + 2 * d) * (tiles[0][1] + 2 * d)), order, -na, word))
    return min(rows)[3] if rows else "none"


def test_halo_tiling_against_enumerated_costs():
    seen = set()
    for oh, ow in itertools.product(list(range(1, 36)) + [40, 41, 48, 56, 64, 68], repeat=2):
        for d in E.DILS:
            for cin, cout, bn, es in ((64, 64, 64, 2), (128, 128, 64, 2), (512, 512, 128, 2), (2048, 512, 256, 2), (128, 128, 128, 1), (512, 512, 256, 1)):
                got = E.halo_tiling(oh, ow, d, cin, cout, f"{'i8' if es == 1 else 'f16'}/{bn}")
                assert got == brute_tiling(oh, ow, d, cin, cout, bn, es), (oh, ow, d, cin, cout, bn, es)
                seen.add(got)
    assert {"16x16", "8x32", "mixed"} <= seen
    # the figures tests/forms.py states: 8 x 32 at the stride-8 map of 64x256, 16 x 16 on its stride-4 map
    assert E.halo_tiling(8, 32, 1, 128, 128, "f16/64") == "8x32" and E.halo_tiling(16, 64, 1, 64, 64, "f16/64") == "16x16"
    assert E.halo_tiling(17, 31, 2, 256, 256, "f16/64") == "mixed"


def test_stem_and_decode_classes():
    for h, w in itertools.product(range(1, 12), repeat=2):
        plan = W.plan(h, w)
        sh, sw = plan[0][3], plan[0][4]
        c = E.stem_classes(h, w, sh, sw)
        assert f"F/frame/{h & 1}{w & 1}" in c and f"F/stem/{sh & 1}{sw & 1}" in c
        # below 7 pixels some window of the stem holds the WHOLE row, clipped on both sides
        whole = [x for x in range(sw) if 2 * x - 3 <= 0 and 2 * x + 3 >= w - 1]
        assert ("F/w/lt7" in c) == bool(whole), (w, whole)
        lh, lw = W.lowres_dims(h, w)
        g = E.decode_classes(w, lh, lw)
        assert ("G/low/h/1" in g) == (lh == 1) and ("G/low/w/1" in g) == (lw == 1) and f"G/w4/{w - 4 * (w // 4)}" in g


def test_layer_classes_by_kind():
    """which families a layer can be in: the GEMM families on every conv but the stem, the 3x3 families on the 3x3 convs, the
    patch-in-LDS and Winograd families on the stride-1 ones, the activation-in-register family on the stride-1 1x1 convs but the logits"""
    for spec, ih, iw, oh, ow in W.plan(146, 215):
        fams = {E.family_of(c) for c in E.layer_classes(spec, ih, iw, oh, ow)}
        if E.is_q_pair_layer(spec):  # the quantised model's layer1: pixel pairs or channel padding, by the width's parity
            assert spec.name.startswith("backbone.layer1.") and spec.cin in (64, 256) and "X/q_pair/pair" in E.layer_classes(spec, ih, iw, oh, ow - ow % 2)
            assert "X/q_pair/padded" in E.layer_classes(spec, ih, iw, oh, ow | 1)
            fams = fams - {"X"} if spec.k == 1 else fams
        if spec.role == "stem":
            assert not fams
        elif spec.k == 3 and spec.stride == 1:
            assert fams == {"A", "B", "C", "D", "X"}, spec.name
        elif spec.k == 3:
            assert fams == {"A", "B"}, spec.name
        elif spec.stride == 1 and spec.role not in ("cls", "auxcls"):
            assert fams == {"A", "E"}, spec.name
        else:
            assert fams == {"A"}, spec.name
    # the image the quantised layer1 kernels see: half the width where it is even (2 x 24 -> 2 x 12: ONE 16 x 16 patch, not 8 x 32)
    l1 = spec_named("backbone.layer1.1.conv2")
    assert E.kernel_dims("i8", l1, 2, 24, 2, 24) == (2, 12, 2, 12) and E.kernel_dims("i8", l1, 2, 25, 2, 25) == (2, 25, 2, 25)
    assert E.kernel_dims("f16", l1, 2, 24, 2, 24) == (2, 24, 2, 24) and E.kernel_dims("i8", spec_named("backbone.layer2.1.conv2"), 2, 24, 2, 24) == (2, 24, 2, 24)
    assert E.halo_tiling(2, 12, 1, 128, 128, "i8/128") == "16x16" and E.halo_tiling(2, 24, 1, 128, 128, "i8/128") == "8x32"
    # the one-row tail of the 256-row forms: the stride-8 map of 146x215 is 19 x 27 = 513 = 2 x 256 + 1
    s = spec_named("backbone.layer3.1.conv1")
    assert E.gemm_classes(s, 19, 27, 256) == {"A/1x1s1/bm256/1"} and E.gemm_classes(s, 31, 33, 256) == {"A/1x1s1/bm256/bm-1"}


# ---- the table of forms and what a profile proves ---------------------------------------------------------------------------------------
def test_forms_table_is_the_librarys():
    t = E.forms_table()
    for mode in F.MODES:
        assert sorted(k for m, k in t if m == mode) == sorted(F.FORMS[mode]), mode
        for cfg, name in F.FORMS[mode].items():
            assert t[(mode, cfg)]["name"] == name
    assert {t[(m, k)]["bm"] for m, k in t if t[(m, k)]["family"] in ("tiled", "hl")} == set(E.BMS)
    assert t[("f32", 6)]["bm"] == 256 and t[("f32", 6)]["bn"] == 128 and t[("f32", 1)]["bm"] == 64
    assert t[("f16", 19)]["family"] == "halo" and t[("f16", 21)]["family"] == "halo4" and t[("i8", 18)]["family"] == "areg"
    assert t[("f16hl", 15)]["family"] == "hl_areg" and t[("f16hl", 17)]["family"] == "hl"


def test_met_classes_from_a_profile():
    """a made-up profile: the form's own kernel on two layers at 146x215, another kernel elsewhere"""
    recs = {"146x215": [("backbone.layer3.1.conv1", "conv_igemm_f32<256,128>", ""), ("backbone.layer3.1.conv2/in", "wino_input", "lds"),
                        ("backbone.layer3.1.conv2", "conv_igemm_f32<128,128>", ""), ("backbone.layer2.0.conv3+downsample", "conv_igemm_f32<256,128>", ""),
                        ("colorcode", "colorcode", "")]}
    met, carried = E.met_classes("f32", 6, False, recs)
    assert carried == {"146x215": ["backbone.layer3.1.conv1", "backbone.layer2.0.conv3"]}
    assert met == {"A/1x1s1/bm256/1", "A/1x1s1/mfma32/1"}
    wide = E.frame_wide_classes(recs, 0)
    assert {"F/frame/01", "G/w4/3", "C/d2/w/mt6/1", "C/d2/h/mt6/other"} <= wide and not any(c.startswith("C/d1") for c in wide)
    halo = {"5x93": [("backbone.layer2.1.conv2", "conv3x3_f16<16x16,128,halo>", "bn64,8x32,na1")]}
    met, _ = E.met_classes("f16", 19, False, halo)
    assert {"D/h/lt16", "D/w/lt16", "X/halo8/h/1", "X/halo8/w/9-15", "D/tile/f16/64/d1/8x32", "B/d1/h/le_d", "B/d1/w/gt_2d"} == met


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-s"]))
