"""Raster without a GPU: the reference of tests/raster_ref.py against its own brute force on hand-made loops, the round trips
through the references of Outlines and Runs, and the mirrors of the new names (header, ctypes, C++, Rust)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import coverage_ref as CV  # noqa: E402
import outlines_ref as O  # noqa: E402
import raster_ref as A  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as RR  # noqa: E402
import simplify_ref as S  # noqa: E402
import stage_limits as SL  # noqa: E402

ROOT = os.path.dirname(HERE)
NONE = 0xFFFFFFFF

HAND_MADE = {
    "diamond": (8, 8, [(7, [(4, 0), (8, 4), (4, 8), (0, 4)])]),
    "triangle": (7, 7, [(3, [(0, 0), (7, 0), (0, 7)])]),
    "two triangles": (6, 6, [(3, [(0, 0), (6, 0), (0, 6)]), (4, [(6, 0), (6, 6), (0, 6)])]),
    "overlap": (10, 12, [(1, A.rect(1, 1, 7, 6)), (2, A.rect(4, 3, 11, 9))]),
    "hole alone": (6, 8, [(1, A.rect(2, 2, 5, 4)[::-1])]),
    "ring": (7, 9, [(5, A.rect(1, 1, 8, 6)), (5, A.rect(3, 2, 6, 5)[::-1])]),
    "too large for a byte": (3, 5, [(300, A.rect(0, 0, 4, 2))]),
    "stacked": (4, 4, [(10, A.rect(0, 0, 4, 4)), (20, A.rect(1, 1, 4, 4)), (7, A.rect(2, 2, 4, 4)[::-1])]),
    "bow tie": (8, 8, [(2, [(0, 0), (8, 8), (8, 0), (0, 8)])]),
    "slanted": (11, 9, [(6, [(1, 1), (6, 0), (8, 10), (2, 7)])]),
    "beyond the right edge": (5, 4, [(1, [(0, 0), (4, 0), (4, 5), (0, 5)])]),
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint32])
def test_reference_against_the_brute_force(name, dtype):
    h, w, polys = HAND_MADE[name]
    l, v, c = A.loops_of(polys, w)
    plane, counts = A.raster(l, v, c, h, w, dtype, 9)
    want, painted, conflict = A.brute(polys, h, w, dtype, 9)
    assert (plane == want).all() and counts.tolist() == [len(polys), painted, conflict, 0]


def test_the_worked_examples():
    plane, counts = A.raster(*A.loops_of(HAND_MADE["diamond"][2], 8), 8, 8)
    assert counts.tolist() == [1, 32, 0, 0]
    assert [int(np.flatnonzero(r)[0]) for r in plane] == [3, 2, 1, 0, 0, 1, 2, 3] and [int(np.flatnonzero(r)[-1]) + 1 for r in plane] == [4, 5, 6, 7, 7, 6, 5, 4]
    plane, counts = A.raster(*A.loops_of(HAND_MADE["overlap"][2], 12), 10, 12, np.uint8, 99)
    assert counts.tolist() == [2, 30 + 42 - 18, 9, 0] and (plane[3:6, 4:7] == 99).all()
    assert A.raster(*A.loops_of(HAND_MADE["hole alone"][2], 8), 6, 8)[1].tolist() == [1, 0, 6, 0]
    assert A.raster(*A.loops_of(HAND_MADE["too large for a byte"][2], 5), 3, 5)[1].tolist() == [1, 0, 8, 0]
    assert A.raster(*A.loops_of(HAND_MADE["stacked"][2], 4), 4, 4)[0][3, 3] == 23  # 10 + 20 - 7: the rule, not a defect
    two = A.raster(*A.loops_of(HAND_MADE["two triangles"][2], 6), 6, 6)
    assert two[1].tolist() == [2, 36, 0, 0]  # the shared diagonal gives each pixel on it to exactly one triangle


@pytest.mark.parametrize("seed", range(8))
def test_round_trips_through_the_references(seed):
    rng = np.random.RandomState(seed)
    h, w = int(rng.randint(1, 14)), int(rng.randint(1, 40))
    plane = rng.randint(0, 3, size=(h, w)).astype(np.uint8)
    for flags in (0, O.CONN8, O.SKIP, O.SKIP | O.CONN8):
        skip = 1 if flags & O.SKIP else 0
        l, v, c = O.outline(plane, flags, skip)
        got, counts = A.raster(l, v, c, h, w, np.uint8, skip if flags & O.SKIP else 200)
        assert (got == plane).all() and counts[A.CONFLICT] == 0 and counts[A.STATUS] == 0, flags
        assert counts[A.PAINTED] == (int((plane != skip).sum()) if flags & O.SKIP else h * w)
    r, _, n = RR.encode(plane, RR.SKIP, 2)
    got, counts = A.raster_runs(r, n, h, w, np.uint8, 2)
    assert (got == plane).all() and counts.tolist() == [n, int((plane != 2).sum()), 0, 0]
    wide = np.where(plane == 0, NONE, plane.astype(np.uint32) + 0xFFFFFFF0).astype(np.uint32)
    l, v, c = O.outline(wide, O.SKIP | O.CONN8, NONE)
    assert (A.raster(l, v, c, h, w, np.uint32, NONE)[0] == wide).all()
    r, _, n = RR.encode(wide)
    assert (A.raster_runs(r, n, h, w, np.uint32, 0)[0] == wide).all()


def test_guards_of_the_reference():
    plane = R.smooth(9, 14, seed=1, classes=3, cell=3)
    l, v, c = O.outline(plane)
    assert A.raster(l, v, c, 9, 14, loops_rows_in=len(l) - 1)[0] is None
    assert A.raster(l, v, c, 9, 14, vertex_rows_in=len(v) - 1)[1].tolist() == [len(l), 0, 0, A.TRUNCATED]
    bad = l.copy()
    bad[0, 1] = 1
    assert A.raster(bad, v, c, 9, 14)[1][A.STATUS] == A.MALFORMED
    far = v.copy()
    far[0] = NONE
    assert A.raster(l, far, c, 9, 14)[1][A.STATUS] & A.OUTSIDE
    runs = np.array([[2, 8, 5], [5, 9, 6], [12, 23, 7], [35, 35, 1]], np.uint32)
    got, counts = A.raster_runs(runs, 4, 4, 10)
    assert counts.tolist() == [4, 3 + 1, 3, A.MALFORMED] and got[0].tolist() == [0, 0, 5, 5, 5, 0, 0, 0, 6, 0]
    assert A.raster_runs(runs, 5, 4, 10)[1].tolist() == [5, 0, 0, A.TRUNCATED]


def test_what_a_tolerance_costs_is_visible():
    """Simplify's arcs of neighbouring loops cross, Coverage's shared borders do not overlap: the reference shows both"""
    plane = R.smooth(48, 80)
    l, v, c = O.outline(plane)
    sl, sv, sc = S.simplify(l, v, c, 80, 16)
    _, counts = A.raster(sl, sv, sc, 48, 80)
    assert counts[A.CONFLICT] > 0 and 48 * 80 - int(counts[A.PAINTED]) - int(counts[A.CONFLICT]) > 0
    cl, cv, cc = CV.coverage(plane, l, v, c, 16)
    _, counts = A.raster(cl, cv, cc, 48, 80)
    assert counts[A.CONFLICT] == 0
    # no tolerance: both are the plane
    for out in (S.simplify(l, v, c, 80, 0), CV.coverage(plane, l, v, c, 0)):
        assert (A.raster(*out[:2], out[2], 48, 80)[0] == plane).all()


def _text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_mirrors_carry_the_new_names():
    header = _text("include", "infur_hip.h")
    names = {"INFUR_RASTER_LOOPS": 0, "INFUR_RASTER_PAINTED": 1, "INFUR_RASTER_CONFLICT": 2, "INFUR_RASTER_STATUS": 3, "INFUR_RASTER_COUNT_WORDS": 4,
             "INFUR_RASTER_TRUNCATED": 1, "INFUR_RASTER_MALFORMED": 2, "INFUR_RASTER_OUTSIDE": 4, "INFUR_FEATURE_RASTER": 4096}
    rust = _text("rust", "infur-hip-sys", "src", "lib.rs")
    from infur_amd import _lib

    for name, value in names.items():
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rust), name
        assert getattr(_lib, name[len("INFUR_"):]) == value, name
    assert re.search(r"#define INFUR_ABI_VERSION 7\b", header)
    for fn in ("infur_raster", "infur_raster_dev", "infur_raster_runs", "infur_raster_runs_dev"):
        assert re.search(r"int32_t %s\(infur_ctx\* ctx," % fn, header), fn
        assert fn in _lib.SIGNATURES and re.search(r"pub fn %s\(" % fn, rust), fn
    hpp = _text("include", "infur_processor.hpp")
    assert "struct RasterOut" in hpp and "class Raster {" in hpp and "infur_raster_runs(" in hpp
    wrapper = _text("rust", "infur-hip", "src", "lib.rs")
    assert "pub struct HipRaster" in wrapper and "impl Processor for HipRaster" in wrapper and "sys::infur_raster_runs(" in wrapper
    assert _lib.load().infur_features() & _lib.FEATURE_RASTER
    from infur_amd import processors

    for name in ("Raster", "RasterCmd", "RasterOut", "polygon_fidelity"):
        assert hasattr(processors, name), name


def test_the_constant_the_edge_forms_turn_on_is_readable():
    rows = SL.constant("raster.hip", "kRasterLaneRows")
    assert 1 <= rows < 64  # a wave has 64 lanes: above that a lane walk is never the cheaper form
    assert SL.constant("raster.hip", "kLoopGrid") * (SL.constant("raster.hip", "kLoopBlock") // 64) == 32768
