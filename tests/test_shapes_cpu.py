"""Shapes (area, moments, convex hull and minimum rectangle per outline loop) without a GPU: the ABI surface, the reference the GPU
tests use (tests/shapes_ref.py) against pixel sums, a brute-force hull and the header's worked examples, a numpy emulation of the
kernels' lane logic against the reference, and ``shape_summary`` against float64 formulas over pixels."""
import ctypes as C
import functools
import itertools
import math
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd.processors import outlines_polygons, shape_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import shapes_ref as H  # noqa: E402
import simplify_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_shapes", "infur_shapes_dev", "infur_frame_shapes", "infur_frame_shapes_dev")
CONSTANTS = {"INFUR_SHAPE_AREA2": 0, "INFUR_SHAPE_PERIMETER": 1, "INFUR_SHAPE_M10_6": 2, "INFUR_SHAPE_M01_6": 3, "INFUR_SHAPE_M20_12": 4,
             "INFUR_SHAPE_M02_12": 5, "INFUR_SHAPE_M11_24": 6, "INFUR_SHAPE_HULL_AREA2": 7, "INFUR_SHAPE_RECT_EDGE": 8, "INFUR_SHAPE_RECT_W": 9,
             "INFUR_SHAPE_RECT_H": 10, "INFUR_SHAPE_RECT_L": 11, "INFUR_SHAPE_WORDS": 12, "INFUR_SHAPE_OUTER": 8, "INFUR_SHAPE_HOLES": 9,
             "INFUR_SHAPE_LOOP": 10, "INFUR_SHAPES_LOOPS": 0, "INFUR_SHAPES_VERTICES": 1, "INFUR_SHAPES_STATUS": 2, "INFUR_SHAPES_LARGEST": 3,
             "INFUR_SHAPES_COUNT_WORDS": 4, "INFUR_SHAPES_TRUNCATED": 1, "INFUR_SHAPES_MALFORMED": 2, "INFUR_FEATURE_SHAPES": 2048}
SKIP, CONN8 = O.SKIP, O.CONN8
SIZES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (40, 70), (135, 241))
SMALL = SIZES[:6]


def families(h, w):
    """the seven families of the sweep"""
    yield "smooth", R.smooth(h, w, seed=h + w)
    yield "noise", R.noise(h, w, 3, seed=w)
    yield "single", R.single(h, w)
    yield "spiral", R.spiral(h, w)
    yield "serpentine", R.serpentine(h, w)
    yield "staircase", R.staircase(h, w)
    yield "checkerboard", R.checkerboard(h, w)


@functools.lru_cache(maxsize=None)
def family_cases(conn, sizes=SIZES):
    """[(name, plane, outline, reference with one row per value)]: computed once, shared, never changed"""
    out = []
    for h, w in sizes:
        for name, k in families(h, w):
            o = O.outline(k, conn)
            out.append((f"{name} {h}x{w}", k, o, H.shapes(*o, w, rows=int(k.max()) + 2)))
    return out


def same(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


# ---------------------------------------------------------------- the ABI surface
def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_SHAPES
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    for older in (_lib.FEATURE_SEGMENTS, _lib.FEATURE_REGIONS, _lib.FEATURE_OUTLINES, _lib.FEATURE_SIMPLIFY, _lib.FEATURE_SIEVE):
        assert lib.infur_features() & older
    assert "pub struct HipShapes" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Shapes" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def test_signatures_count_the_header_s_parameters():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    for s in NEW_SYMBOLS:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[s][1]), s
    # infur_shapes is infur_simplify without tol16 and with two more tables; the frame call is infur_frame_regions plus nine
    assert len(_lib.SIGNATURES["infur_shapes_dev"][1]) == len(_lib.SIGNATURES["infur_simplify_dev"][1]) - 1 + 4
    for s in ("", "_dev"):
        assert len(_lib.SIGNATURES["infur_frame_shapes" + s][1]) == len(_lib.SIGNATURES["infur_frame_regions" + s][1]) + 9


def test_constants_agree_in_header_binding_crate_and_reference():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert (H.STATUS_TRUNCATED, H.STATUS_MALFORMED) == (_lib.SHAPES_TRUNCATED, _lib.SHAPES_MALFORMED)
    assert [H.AREA2, H.M11_24, H.HULL_AREA2, H.RECT_EDGE, H.RECT_L, H.SHAPE_WORDS] == [_lib.SHAPE_AREA2, _lib.SHAPE_M11_24, _lib.SHAPE_HULL_AREA2,
                                                                                         _lib.SHAPE_RECT_EDGE, _lib.SHAPE_RECT_L, _lib.SHAPE_WORDS]
    assert (H.OUTER, H.HOLES, H.LOOP) == (_lib.SHAPE_OUTER, _lib.SHAPE_HOLES, _lib.SHAPE_LOOP)


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else and no output is touched"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_shapes(None, p, 1, p, 4, p, 2, 2, p, 1, p, 4, p, 1, p, 1, p) == _lib.E_INVALID_ARG
    assert lib.infur_shapes_dev(None, p, 1, p, 4, p, 2, 2, p, 1, p, 4, p, 1, p, 1, p) == _lib.E_INVALID_ARG
    frame = (p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, None, 0, None, 0, None, None, C.byref(ow), C.byref(oh), 0, p, 1, p, 4, p, 1, None, p)
    assert lib.infur_frame_shapes(None, *frame) == _lib.E_INVALID_ARG and lib.infur_frame_shapes_dev(None, *frame) == _lib.E_INVALID_ARG
    assert (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


# ---------------------------------------------------------------- the reference against the issue's facts
def test_worked_example_1_the_c():
    plane = H.letter_c()
    l, v, c = O.outline(plane, SKIP, 0)
    assert c.tolist()[:2] == [1, 8]
    x, y = S._xy(v, 24)
    assert list(zip(x, y)) == [(2, 2), (22, 2), (22, 7), (7, 7), (7, 17), (22, 17), (22, 22), (2, 22)]
    lo, vo, sh, vals, cnt = H.shapes(l, v, c, 24, rows=2)
    assert sh[0].tolist() == [500, 110, 15750, 18000, 439000, 577000, 756000, 800, 0, 400, 400, 400]
    assert list(zip(*H.hull_xy(lo, vo, 0, 24))) == [(2, 2), (22, 2), (22, 22), (2, 22)]
    assert lo.tolist() == [[0, 4, 1, int(l[0, 3])]] and cnt.tolist() == [1, 4, 0, 4]
    assert vals[1].tolist() == [500, 110, 15750, 18000, 439000, 577000, 756000, 800, 1, 0, 0, 0] and vals[0].tolist() == [0] * 10 + [-1, 0]
    s = shape_summary(sh[0], sh[0], np.array(H.hull_xy(lo, vo, 0, 24)).T)
    assert s["solidity"] == 0.625 and s["centroid"][0] == 10.0 and s["area"] == 250 and s["rect_sides"] == (20.0, 20.0)
    assert s["rect_centre"] == (11.5, 11.5) and s["rect_angle"] == 0.0


def test_worked_example_2_the_slanted_bar():
    plane = H.bar()
    assert plane.shape == (12, 16)
    l, v, c = O.outline(plane, SKIP, 0)
    assert c.tolist()[:2] == [1, 40]
    lo, vo, sh, vals, cnt = H.shapes(l, v, c, 16, rows=3)
    assert sh[0].tolist() == [60, 44, 1440, 1080, 26280, 15960, 40500, 78, 1, 198, 36, 162]
    assert list(zip(*H.hull_xy(lo, vo, 0, 16))) == [(2, 1), (5, 1), (14, 10), (14, 11), (11, 11), (2, 2)]
    assert vals[2, :8].tolist() == sh[0, :8].tolist() and vals[2, H.LOOP] == 0
    s = shape_summary(vals[2], sh[0])
    assert s["rect_sides"] == pytest.approx((15.556349186104045, 2.8284271247461903), rel=1e-12)
    assert s["rect_sides"][0] * s["rect_sides"][1] == pytest.approx(44.0, rel=1e-12)


@pytest.mark.parametrize("r, n, k, rect", [(10, 52, 24, (1, 85, 85, 17)), (40, 196, 48, (1, 649, 649, 65)), (120, 572, 88, (11, 5100, 5100, 450))])
def test_discs(r, n, k, rect):
    plane = H.disc(r)
    assert plane.shape == (2 * r + 3, 2 * r + 3)
    l, v, c = O.outline(plane, SKIP, 0)
    lo, vo, sh, _, cnt = H.shapes(l, v, c, plane.shape[1])
    assert c.tolist()[:2] == [1, n] and cnt.tolist() == [1, k, 0, k] and tuple(sh[0, 8:].tolist()) == rect
    got = H.emulate(l, v, c, plane.shape[1])  # more than 64 hull vertices at r = 120: the rectangle's second stride
    assert same(got, (lo, vo, sh, np.zeros((0, 12), np.int64), cnt))


@pytest.mark.parametrize("conn", [0, CONN8])
def test_per_value_sums_equal_the_pixel_sums(conn):
    loops = 0
    for name, k, (l, v, c), (lo, vo, sh, vals, cnt) in family_cases(conn):
        loops += int(c[0])
        assert cnt[2] == 0 and cnt[0] == c[0], name
        for value in range(len(vals)):
            want = H.pixel_sums(k == value)
            assert [int(vals[value, j]) for j in (H.AREA2, H.M10_6, H.M01_6, H.M20_12, H.M02_12, H.M11_24)] == want, (name, value)
            outer = [i for i in range(len(l)) if l[i, 2] == value and sh[i, H.AREA2] > 0]
            assert vals[value, H.OUTER] == len(outer) and vals[value, H.HOLES] == int((l[:, 2] == value).sum()) - len(outer)
            assert vals[value, H.HULL_AREA2] == sum(int(sh[i, H.HULL_AREA2]) for i in outer)
            if outer:
                top = max(int(sh[i, H.AREA2]) for i in outer)
                assert vals[value, H.LOOP] == min(i for i in outer if sh[i, H.AREA2] == top)
            else:
                assert vals[value, H.LOOP] == -1
        # the Euler number of a value is its regions minus its holes: 8-connected regions under CONN8, 4-connected otherwise
        H.check_invariants(l, v, k.shape[1], lo, vo, sh)
    print(f"conn {conn}: {loops} loops")
    assert loops > 20000


def brute_force_hull(pts):
    """a point is extreme iff it lies in no triangle (or on no segment) of the others"""
    pts = sorted(set(pts))
    out = set()
    for p in pts:
        others = [q for q in pts if q != p]
        inside = False
        for a, b in itertools.combinations(others, 2):  # on the closed segment a b
            if H._cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1]):
                inside = True
                break
        if not inside:
            for a, b, c in itertools.combinations(others, 3):
                d = [H._cross(a, b, p), H._cross(b, c, p), H._cross(c, a, p)]
                if H._cross(a, b, c) != 0 and (all(t >= 0 for t in d) or all(t <= 0 for t in d)):
                    inside = True
                    break
        if not inside:
            out.add(p)
    return out


def test_the_monotone_chain_equals_a_brute_force_hull_on_small_planes():
    checked = 0
    for h, w in ((1, 1), (1, 5), (5, 1), (3, 64), (7, 9), (6, 11)):
        for name, k in families(h, w):
            for conn in (0, CONN8):
                l, v, c = O.outline(k, conn)
                for off, cnt, _, _ in l.tolist():
                    if cnt > 28:
                        continue
                    x, y = S._xy(v[off:off + cnt], w)
                    kept = H.hull_indices(x, y)
                    assert {(x[i], y[i]) for i in kept} == brute_force_hull(list(zip(x, y))), (name, h, w, off)
                    checked += 1
    assert checked > 300


# ---------------------------------------------------------------- the lane emulation against the reference
@pytest.mark.parametrize("conn", [0, CONN8])
def test_the_lane_emulation_equals_the_reference_on_the_families(conn):
    for name, k, (l, v, c), ref in family_cases(conn):
        if k.size > 40 * 70 and not name.startswith(("smooth", "spiral", "serpentine", "single")):
            continue  # (the dense families at 135 x 241 are thousands of unit squares: the smaller sizes walk the same lanes)
        got = H.emulate(l, v, c, k.shape[1], rows=int(k.max()) + 2)
        assert same(got, ref), name


def hand_made():
    """[(name, (loops, vertices, counts), w)]: loops no family has"""
    out = []
    for kk in (3, 30, 31, 32, 63, 64, 100):
        plane = S.stairs(kk)
        out.append((f"stairs {kk}", O.outline(plane, SKIP, 0), kk))
    comb = S.comb(40, 200)
    out.append(("comb", O.outline(comb, SKIP, 0), 200))
    for n in (4, 63, 64, 65, 129):
        out.append((f"polygon {n}", H.loop_of(H.polygon_of(n), 80), 80))
    for n, turn in ((65, 1), (65, 40), (129, 64), (129, 127), (64, 63)):  # begun anywhere: either anchor may come first, both ranges wrap
        pts = H.polygon_of(n)
        out.append((f"turned {n} by {turn}", H.loop_of(pts[turn:] + pts[:turn], 80), 80))
        out.append((f"turned back {n} by {turn}", H.loop_of((pts[turn:] + pts[:turn])[::-1], 80), 80))
    out.append(("annulus", O.outline(H.annulus(20, 9), SKIP, 0), 43))
    out.append(("annulus conn8", O.outline(H.annulus(9, 4), SKIP | CONN8, 0), 21))
    return out


def test_the_lane_emulation_on_hand_made_loops():
    for name, (l, v, c), w in hand_made():
        ref = H.shapes(l, v, c, w, rows=3)
        got = H.emulate(l, v, c, w, rows=3)
        assert same(got, ref), name
        if name.startswith("polygon"):
            n = int(name.split()[1])
            # the hull is (0,0) (1,0) (k,k-1) (k,k) (0,k) (the unit square at n = 4): the collinear vertex of an odd n is dropped
            assert c[1] == n and ref[4][1] == (4 if n == 4 else 5)
    l, v, c = O.outline(H.annulus(20, 9), SKIP, 0)
    lo, vo, sh, vals, cnt = H.shapes(l, v, c, 43, rows=2)
    assert len(l) == 2 and sh[1, H.AREA2] < 0 and sh[1, H.HULL_AREA2] < sh[1, H.AREA2] < 0  # the hole: its sign throughout
    assert vals[1, H.OUTER] == 1 and vals[1, H.HOLES] == 1 and vals[1, H.LOOP] == 0 and vals[1, H.AREA2] == 2 * int(H.annulus(20, 9).sum())
    x, y = S._xy(v[l[1, 0]:l[1, 0] + l[1, 1]], 43)
    assert min(zip(y, x)) != (y[0], x[0])  # the hole does not start at its first anchor: the kernel's ranges wrap past n


def test_the_largest_square_and_the_diagonal_staircase():
    l, v, c = H.loop_of([(0, 0), (8191, 0), (8191, 8191), (0, 8191)], 8191)
    ref = H.shapes(l, v, c, 8191, rows=2)
    assert ref[2][0, H.M20_12] == 4 * 8191 ** 4 and ref[2][0, H.M11_24] == 6 * 8191 ** 4 and ref[2][0, 8:].tolist() == [0, 8191 ** 2, 8191 ** 2, 8191 ** 2]
    assert same(H.emulate(l, v, c, 8191, rows=2), ref)
    pts = H.diagonal_staircase(8000)
    l, v, c = H.loop_of(pts, 8191)
    assert len(pts) == 16002
    ref = H.shapes(l, v, c, 8191, rows=2)
    x, y = [p[0] for p in pts], [p[1] for p in pts]
    assert 3 <= ref[4][1] <= 8 and [int(t) for t in ref[2][0, :7]] == H.measures(x, y)  # the true values fit; steps of 1 and 2 leave a few corners
    m, kept = H.hull_loop_lanes(x, y)  # the lanes' sums wrap at 64 bits on the way: a negative c is a large unsigned word
    assert [H.signed64(t) for t in m] == H.measures(x, y) and kept == H.hull_indices(x, y)


def test_the_lane_emulation_on_truncated_and_malformed_input():
    k = R.smooth(65, 130)
    l, v, c = O.outline(k)
    nl, nv = len(l), len(v)
    for lin, vin in ((nl - 1, nv), (nl, nv - 1), (1, 1), (0, nv), (nl, 0), (0, 0)):
        ref = H.shapes(l, v, c, 130, rows=4, loops_rows_in=lin, vertex_rows_in=vin)
        got = H.emulate(l, v, c, 130, rows=4, loops_rows_in=lin, vertex_rows_in=vin, loops_rows_out=0, vertex_rows_out=0, shape_rows=0)
        assert ref[4].tolist() == got[4].tolist() == [nl, 0, 1, 0] and (got[3] == ref[3]).all() and (ref[3][:, H.LOOP] == -1).all()
    bad = l.copy()
    bad[2, 1] = 1
    bad[5, 1] = 0
    bad[nl - 1, 1] += 3
    bad[nl - 3, 0], bad[nl - 3, 1] = nv + 9, 4
    ref = H.shapes(bad, v, c, 130, rows=21)
    assert ref[4][2] == H.STATUS_MALFORMED and (ref[0][[2, 5, nl - 1, nl - 3], 1] == 0).all() and (ref[2][[2, 5, nl - 1, nl - 3]] == 0).all()
    assert same(H.emulate(bad, v, c, 130, rows=21), ref)
    good = H.shapes(l, v, c, 130, rows=21)
    keep = np.ones(nl, bool)
    keep[[2, 5, nl - 1, nl - 3]] = False
    assert (ref[2][keep] == good[2][keep]).all()  # the well-formed loops are described as ever
    # short output rows: the full prefix sums and counts, the rest poisoned
    got = H.emulate(l, v, c, 130, rows=2, loops_rows_out=3, vertex_rows_out=5, shape_rows=4)
    assert (got[0] == good[0][:3]).all() and (got[1] == good[1][:5]).all() and (got[2] == good[2][:4]).all() and got[4].tolist() == good[4].tolist()
    assert (got[3] == good[3][:2]).all()


# ---------------------------------------------------------------- shape_summary
def test_shape_summary_equals_the_formulas_over_pixels_in_float64():
    """The inputs are exact integers below 2^40 on these planes; what separates the two sides is double rounding through one
    subtraction: relative 1e-9.  (An angle is compared on the scale of a radian.)"""
    planes = [("bar", H.bar() == 2), ("c", H.letter_c() == 1), ("disc", H.disc(10) == 1), ("annulus", H.annulus(20, 9) == 1),
              ("smooth", R.smooth(33, 63, seed=96) == R.smooth(33, 63, seed=96)[16, 31])]
    for name, mask in planes:
        plane = mask.astype(np.uint8)
        l, v, c = O.outline(plane, SKIP | CONN8, 0)
        lo, vo, sh, vals, cnt = H.shapes(l, v, c, plane.shape[1], rows=2)
        s = shape_summary(vals[1], sh[vals[1, H.LOOP]], np.array(H.hull_xy(lo, vo, int(vals[1, H.LOOP]), plane.shape[1])).T)
        ys, xs = np.nonzero(mask)
        xs, ys = xs.astype(np.float64), ys.astype(np.float64)
        n = float(len(xs))
        cx, cy = xs.sum() / n, ys.sum() / n
        mu20 = ((xs + 0.5) ** 2).sum() + n / 12 - n * (cx + 0.5) ** 2
        mu02 = ((ys + 0.5) ** 2).sum() + n / 12 - n * (cy + 0.5) ** 2
        mu11 = ((xs + 0.5) * (ys + 0.5)).sum() - n * (cx + 0.5) * (cy + 0.5)
        root = math.hypot(mu20 - mu02, 2 * mu11)
        big, small = (mu20 + mu02 + root) / (2 * n), (mu20 + mu02 - root) / (2 * n)
        assert s["area"] == n and s["perimeter"] == float(vals[1, H.PERIMETER])
        assert s["centroid"] == pytest.approx((cx, cy), rel=1e-9), name
        assert s["orientation"] == pytest.approx(0.5 * math.atan2(2 * mu11, mu20 - mu02), rel=1e-9, abs=1e-9), name
        assert s["major"] == pytest.approx(4 * math.sqrt(big), rel=1e-9) and s["minor"] == pytest.approx(4 * math.sqrt(small), rel=1e-9), name
        assert s["eccentricity"] == pytest.approx(math.sqrt(1 - small / big), rel=1e-9, abs=1e-9), name
        assert s["solidity"] == pytest.approx(2 * n / float(vals[1, H.HULL_AREA2]), rel=1e-9), name
        assert s["compactness"] == pytest.approx(4 * math.pi * n / float(vals[1, H.PERIMETER]) ** 2, rel=1e-9), name
        w, hh, length = (float(t) for t in sh[vals[1, H.LOOP], 9:])
        assert s["rect_sides"] == pytest.approx((w / math.sqrt(length), hh / math.sqrt(length)), rel=1e-9), name
    assert shape_summary(np.zeros(12, np.int64)) is None
    # the hulls read like Outlines' loops
    l, v, c = O.outline(H.bar(), SKIP, 0)
    lo, vo, *_ = H.shapes(l, v, c, 16)
    assert [p[2].tolist() for p in outlines_polygons(lo, vo, 16)] == [[[2, 1], [5, 1], [14, 10], [14, 11], [11, 11], [2, 2]]]


def test_rate_script_tables_without_a_device(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import shapes_rate

    shapes_rate.main(["--tables", "--height", "135", "--width", "241"])
    out = capsys.readouterr().out
    assert "smooth" in out and "hull vertices" in out
