"""Simplify (Douglas-Peucker on Outlines' loops) without a GPU: the ABI surface, the reference the GPU tests use
(tests/simplify_ref.py) against its own invariants and pinned numbers, and a numpy emulation of the kernels' lane logic."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd.processors import SimplifyCmd, outlines_by_value, outlines_polygons, tolerance_to_tol16

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import simplify_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_simplify", "infur_simplify_dev", "infur_frame_polygons", "infur_frame_polygons_dev")
CONSTANTS = {"INFUR_SIMPLIFY_LOOPS": 0, "INFUR_SIMPLIFY_VERTICES": 1, "INFUR_SIMPLIFY_DEGENERATE": 2, "INFUR_SIMPLIFY_STATUS": 3,
             "INFUR_SIMPLIFY_COUNT_WORDS": 4, "INFUR_SIMPLIFY_TRUNCATED": 1, "INFUR_SIMPLIFY_MALFORMED": 2, "INFUR_FEATURE_SIMPLIFY": 32}
SKIP, CONN8 = O.SKIP, O.CONN8
TOLS = (0, 8, 11, 12, 16, 32, 4096, 65535)
SMALL_SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63))


def families(h, w):
    """the nine families of tests/test_gpu_outlines.py"""
    yield "smooth", R.smooth(h, w, seed=h + w)
    yield "noise2", R.noise(h, w, 2, seed=w)
    yield "noise21", R.noise(h, w, 21, seed=h)
    yield "single", R.single(h, w)
    yield "vstripes", R.stripes(h, w, vertical=True)
    yield "hstripes", R.stripes(h, w, vertical=False)
    yield "checkerboard", R.checkerboard(h, w)
    yield "staircase", R.staircase(h, w)
    yield "snake", O.snake(h, w)


def same(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_SIMPLIFY
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    for older in (_lib.FEATURE_SEGMENTS, _lib.FEATURE_REGIONS, _lib.FEATURE_TRACKS, _lib.FEATURE_RUNS, _lib.FEATURE_OUTLINES):  # the five older bits
        assert lib.infur_features() & older
    assert "pub struct HipSimplify" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Simplify" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def test_signatures_count_the_header_s_parameters():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    for s in NEW_SYMBOLS:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[s][1]), s
    # infur_frame_polygons is infur_frame_outlines plus tol16
    for s in ("", "_dev"):
        assert len(_lib.SIGNATURES["infur_frame_polygons" + s][1]) == len(_lib.SIGNATURES["infur_frame_outlines" + s][1]) + 1


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert (S.STATUS_TRUNCATED, S.STATUS_MALFORMED) == (_lib.SIMPLIFY_TRUNCATED, _lib.SIMPLIFY_MALFORMED)
    assert (S.OFFSET, S.COUNT, S.VALUE, S.START, S.WORDS) == (_lib.LOOP_OFFSET, _lib.LOOP_COUNT, _lib.LOOP_VALUE, _lib.LOOP_START, _lib.LOOP_WORDS)


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else and no output is touched"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_simplify(None, p, 1, p, 4, p, 2, 2, 16, p, 1, p, 4, p) == _lib.E_INVALID_ARG
    assert lib.infur_simplify_dev(None, p, 1, p, 4, p, 2, 2, 16, p, 1, p, 4, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_polygons(None, p, 4, 4, 1.0, 0, 0, 0, 0, 0, 16, p, 4, p, 16, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert lib.infur_frame_polygons_dev(None, p, 4, 4, 1.0, 0, 0, 0, 0, 0, 16, p, 4, p, 16, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


def test_tolerance_rounds_to_sixteenths():
    assert [tolerance_to_tol16(px) for px in (0, 0.03, 0.5, 0.7, 0.75, 1, 2, 4095.9)] == [0, 0, 8, 11, 12, 16, 32, 65534]
    assert SimplifyCmd.Tolerance(0.6875).tol16 == 11
    for bad in (-0.1, 4096.0):
        with pytest.raises(Exception):
            tolerance_to_tol16(bad)


# ---------------------------------------------------------------- the reference against hand-written answers
def test_reference_on_hand_written_loops():
    # a 4 x 2 rectangle: the anchors are a diagonal; corner (4, 0) has cross = -8, D = 64 against L = 20:
    # 256 * 64 > tol16^2 * 20 up to tol16 = 28 (1.79 px is 28.6 sixteenths)
    l, v, c = O.outline(np.ones((2, 4), np.uint8))
    assert v.tolist() == [0, 4, 14, 10]
    for tol16, want in ((0, [0, 4, 14, 10]), (28, [0, 4, 14, 10]), (29, [0, 14])):
        lo, vo, co = S.simplify(l, v, c, 4, tol16)
        assert vo.tolist() == want and lo.tolist() == [[0, len(want), 1, 0]] and co.tolist() == [1, len(want), int(len(want) < 3), 0], tol16
    # three unit steps: (0,0) (1,0) (1,1) (2,1) (2,2) (3,2) (3,3) (0,3).  B = 6.  On the chord 0 -> 6 the outer corners 1, 3, 5 tie
    # with D = 9 against L = 18 (0.707 px): the smallest index, 1, is examined.  At tol16 = 11, 2304 > 2178: vertex 1 is kept, and on
    # the chord 1 -> 6 (L = 13) the largest D is 4: 1024 <= 1573, nothing more.  At tol16 = 12, 2304 <= 2592: the staircase is its chord.
    # Vertex 7 has D = 81 against L = 18 on the chord 6 -> 0: kept up to tol16 = 33
    l, v, c = O.outline(S.stairs(3), SKIP, 0)
    assert c.tolist()[:2] == [1, 8] and O.polygons(l, v, 3)[0][2] == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (0, 3)]
    x, y = S._xy(v, 3)
    assert S.keep_loop(x, y, 0) == list(range(8)) and S.keep_loop(x, y, 11) == [0, 1, 6, 7]
    assert S.keep_loop(x, y, 12) == [0, 6, 7] == S.keep_loop(x, y, 33) and S.keep_loop(x, y, 34) == [0, 6]
    assert [a.tolist() for a in S.simplify(l, v, c, 3, 12)] == [[[0, 3, 1, 0]], [0, 15, 12], [1, 3, 0, 0]]
    # ties in the anchor resolve to the smallest index: from (0,0), vertices 1 = (5,0) and 3 = (0,5) are equally far
    assert S.keep_loop([0, 5, 1, 0], [0, 0, 1, 5], 65535) == [0, 1] and S.keep_loop([0, 0, 1, 5], [0, 5, 1, 0], 65535) == [0, 1]
    assert S.keep_loop([0, 1, 1, 0], [0, 0, 1, 1], 12) == [0, 2]  # the unit square: the diagonal


def test_reference_on_a_self_touching_loop():
    """the saddle under 8-connectivity: one loop of 8 vertices that passes vertex (1, 1) twice, as vertices 2 and 6"""
    l, v, c = O.outline(np.array([[1, 0], [0, 1]], np.uint8), SKIP | CONN8, 0)
    assert v.tolist() == [0, 1, 4, 5, 8, 7, 4, 3]
    x, y = S._xy(v, 2)
    assert S.keep_loop(x, y, 0) == list(range(8)) and S.keep_loop(x, y, 11) == [0, 1, 4, 5] and S.keep_loop(x, y, 12) == [0, 4]
    lo, vo, co = S.simplify(l, v, c, 2, 12)
    S.check_invariants(l, v, c, 2, 12, lo, vo, co)
    assert co.tolist() == [1, 2, 1, 0]
    # L == 0 needs a segment whose ends coincide.  A vertex the rule keeps has D > 0 against its chord, so it differs from both
    # ends, and B differs from v_0 unless every vertex is the same point: only such a loop -- no plane has one -- takes that
    # branch, with D = 0 everywhere.  It keeps its anchors 0 and 1
    for n in (2, 3, 70, 200):
        assert S.keep_loop([3] * n, [2] * n, 0) == [0, 1] == S.keep_loop_lanes([3] * n, [2] * n, 0)
    ids = np.full(70, 2 * 10 + 3, np.uint32)
    lo, vo, co = S.simplify(np.array([[0, 70, 1, 0]], np.uint32), ids, [1, 70], 9, 0)
    assert lo.tolist() == [[0, 2, 1, 0]] and vo.tolist() == [23, 23] and co.tolist() == [1, 2, 1, 0]
    assert same(S.emulate(np.array([[0, 70, 1, 0]], np.uint32), ids, [1, 70], 9, 0), (lo, vo, co))
    # a hand-made loop that doubles back through a point: every segment still has distinct ends
    x, y = [0, 4, 4, 4, 8, 4], [0, 0, 1, 0, 0, -9]
    assert S.keep_loop(x, y, 15) == [0, 1, 2, 3, 4, 5] and S.keep_loop(x, y, 16) == [0, 4, 5]  # vertex 2: D = 64 against L = 64
    assert S.keep_loop_lanes(x, y, 15) == [0, 1, 2, 3, 4, 5] and S.keep_loop_lanes(x, y, 16) == [0, 4, 5]


def test_pinned_facts():
    """a change of the rule must change these numbers on purpose"""
    k = R.smooth(270, 480, seed=750)
    l, v, c = O.outline(k)
    assert c.tolist()[:2] == [534, 21244]
    lo, vo, co = S.simplify(l, v, c, 480, 0)
    assert co.tolist() == [534, 21244, 0, 0] and (vo == v).all() and (lo == l).all()  # Outlines leaves nothing collinear along a chord here
    for tol16, n_vertices, n_degenerate in ((11, 11466, 0), (12, 8454, 55), (16, 4421, 76), (32, 2859, 104)):
        lo, vo, co = S.simplify(l, v, c, 480, tol16)
        assert co.tolist() == [534, n_vertices, n_degenerate, 0], tol16
        S.check_invariants(l, v, c, 480, tol16, lo, vo, co)
    for h, w in ((7, 65), (65, 130), (270, 480)):  # (a rectangle loses its other two corners only at h*w / sqrt(h^2 + w^2) px)
        ls, vs, cs = O.outline(R.single(h, w))
        for tol16 in (0, 8, 11, 12, 16, 32):
            assert S.simplify(ls, vs, cs, w, tol16)[2].tolist() == [1, 4, 0, 0], (h, w, tol16)  # `single` stays at 4 vertices


@pytest.mark.parametrize("conn", [0, CONN8])
def test_invariants_idempotence_and_the_lane_emulation_on_the_families(conn):
    """the sequential rule, its invariants, simplify(simplify(x)) == simplify(x), and the kernels' lane logic in numpy"""
    for h, w in SMALL_SHAPES:
        for name, k in families(h, w):
            l, v, c = O.outline(k, conn)
            for tol16 in TOLS:
                ref = S.simplify(l, v, c, w, tol16)
                S.check_invariants(l, v, c, w, tol16, *ref)
                assert same(S.simplify(ref[0], ref[1], ref[2], w, tol16)[:2], ref[:2]), (name, h, w, tol16)
                lanes = S.emulate(l, v, c, w, tol16)
                assert same(lanes, ref), (name, h, w, conn, tol16)
                # the helpers of the package read the simplified arrays as they read Outlines'
                if tol16 == 16 and h * w < 500:
                    polys = outlines_polygons(ref[0], ref[1], w)
                    assert [len(p[2]) for p in polys] == ref[0][:, S.COUNT].tolist()
                    assert sorted(outlines_by_value(ref[0], ref[1], w)) == sorted(outlines_by_value(l, v, w))


def test_the_lane_emulation_on_wave_edges_truncations_and_malformed_records():
    for n_vertices in (62, 64, 66, 126, 128, 130):
        k = (n_vertices - 2) // 2
        l, v, c = O.outline(S.stairs(k), SKIP, 0)
        assert c.tolist()[:2] == [1, n_vertices]
        for tol16 in TOLS:
            assert same(S.emulate(l, v, c, k, tol16), S.simplify(l, v, c, k, tol16)), (n_vertices, tol16)
    plane = R.smooth(33, 63, seed=96)
    l, v, c = O.outline(plane)
    nl, nv = len(l), len(v)
    assert nl > 8
    for tol16 in (0, 12, 32):
        ref = S.simplify(l, v, c, 63, tol16)
        rl, rv, rc = ref
        # a small scan block: several block sums, as on the device with 1024
        assert same(S.emulate(l, v, c, 63, tol16, block=64), ref)
        # truncated outputs: OFFSET' stays the full prefix sum
        for lrows, vrows in ((0, nv), (1, nv), (nl - 1, nv), (nl, 0), (nl, 1), (nl, len(rv) - 1), (nl + 7, nv + 7), (1, 1)):
            lo, vo, co = S.emulate(l, v, c, 63, tol16, loops_rows_out=lrows, vertex_rows_out=vrows)
            ml, mv = min(nl, lrows), min(len(rv), vrows)
            assert co.tolist() == rc.tolist() and (lo[:ml] == rl[:ml]).all() and (lo[ml:] == 0xA5A5A5A5).all()
            assert (vo[:mv] == rv[:mv]).all() and (vo[mv:] == 0xA5A5A5A5).all()
        # truncated input: status bit 0, nothing but the counts
        for lin, vin in ((nl - 1, nv), (nl, nv - 1), (0, 0)):
            lo, vo, co = S.emulate(l, v, c, 63, tol16, lin, vin, nl, nv)
            assert co.tolist() == [nl, 0, 0, 1] == S.simplify(l, v, c, 63, tol16, lin, vin)[2].tolist()
            assert (lo == 0xA5A5A5A5).all() and (vo == 0xA5A5A5A5).all()
        # malformed records: status bit 1, COUNT' = 0, the others as ever
        bad = l.copy()
        bad[2, S.COUNT] = 1
        bad[4, S.COUNT] = 0
        bad[nl - 1, S.COUNT] += 3
        bad[nl - 3, S.OFFSET], bad[nl - 3, S.COUNT] = nv + 9, 4
        bad[1, S.OFFSET], bad[1, S.COUNT] = 0xFFFFFFFE, 6  # a sum that wraps around 2^32 is malformed, not small
        ref = S.simplify(bad, v, c, 63, tol16)
        assert ref[2][3] == 2 and (ref[0][[1, 2, 4, nl - 1, nl - 3], S.COUNT] == 0).all() and ref[2][2] >= 5
        assert same(S.emulate(bad, v, c, 63, tol16), ref)
        keep = np.ones(nl, bool)
        keep[[1, 2, 4, nl - 1, nl - 3]] = False
        assert (ref[0][keep][:, S.COUNT] == rl[keep][:, S.COUNT]).all()


def test_the_comb_plane_is_one_long_loop():
    """(what the plane is for; no device needed to say it)"""
    l, v, c = O.outline(S.comb(130, 2100), SKIP, 0)
    assert c[0] == 1 and c[1] > 1 << 16
    small = S.comb(20, 100)
    l, v, c = O.outline(small, SKIP, 0)
    assert c[0] == 1
    for tol16 in (11, 16, 32):
        ref = S.simplify(l, v, c, 100, tol16)
        S.check_invariants(l, v, c, 100, tol16, *ref)
        assert same(S.emulate(l, v, c, 100, tol16, block=64), ref)


def test_rate_script_tables_without_a_device(capsys):
    """scripts/simplify_rate.py imports, generates its planes and formats both tables (made-up times: only the code path is checked)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("simplify_rate", os.path.join(ROOT, "scripts", "simplify_rate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dry-run"])
    lines = capsys.readouterr().out.splitlines()
    rows = [line for line in lines if line.startswith("| smooth") or line.startswith("| one class") or line.startswith("| noise") or line.startswith("| comb")]
    assert len(rows) == 4 * 3  # four planes at tol16 11, 16, 32
    assert all(line.count("|") >= 9 for line in rows)
    assert sum(line.startswith("| infur_frame_") for line in lines) == 2
    k = R.smooth(54, 96)
    l, v, c = O.outline(k)
    n = int(S.simplify(l, v, c, 96, 16)[2][1])
    assert f"| smooth 54x96 | 16 | {int(c[0])} | {int(c[1])} | {n} |" in "\n".join(lines)
