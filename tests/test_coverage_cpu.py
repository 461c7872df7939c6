"""Coverage (shared borders simplified once) without a GPU: the ABI surface, and the reference the GPU tests use
(tests/coverage_ref.py) against what the stage guarantees, hand-written answers and the figures it was specified with."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib, segments_cli

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_ref as V  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import simplify_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_coverage", "infur_coverage_dev", "infur_frame_coverage", "infur_frame_coverage_dev")
CONSTANTS = {"INFUR_COVERAGE_SKIP": 1, "INFUR_COVERAGE_LOOPS": 0, "INFUR_COVERAGE_VERTICES": 1, "INFUR_COVERAGE_DEGENERATE": 2,
             "INFUR_COVERAGE_STATUS": 3, "INFUR_COVERAGE_AUG": 4, "INFUR_COVERAGE_ARCS": 5, "INFUR_COVERAGE_COUNT_WORDS": 6,
             "INFUR_COVERAGE_TRUNCATED": 1, "INFUR_COVERAGE_MALFORMED": 2, "INFUR_COVERAGE_OVERFLOW": 4, "INFUR_FEATURE_COVERAGE": 64}
CONN8 = O.CONN8
TOLS = (0, 11, 12, 16, 64, 65535)


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_COVERAGE
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    assert lib.infur_features() & 63 == 63  # the six older bits
    assert "pub struct HipCoverage" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Coverage" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def test_signatures_count_the_header_s_parameters():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    for s in NEW_SYMBOLS:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[s][1]), s
    for s in ("", "_dev"):  # the frame calls are the twins of infur_frame_polygons
        assert _lib.SIGNATURES["infur_frame_coverage" + s] == _lib.SIGNATURES["infur_frame_polygons" + s]


def test_constants_agree_in_header_binding_reference_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert (V.STATUS_TRUNCATED, V.STATUS_MALFORMED, V.STATUS_OVERFLOW) == (_lib.COVERAGE_TRUNCATED, _lib.COVERAGE_MALFORMED, _lib.COVERAGE_OVERFLOW)
    assert (V.SKIP, V.COUNT_WORDS) == (_lib.COVERAGE_SKIP, _lib.COVERAGE_COUNT_WORDS)


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else and no output is touched"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_coverage(None, p, 1, 2, 2, 0, 0, p, 1, p, 4, p, 16, 0, p, 1, p, 4, p) == _lib.E_INVALID_ARG
    assert lib.infur_coverage_dev(None, p, 1, 2, 2, 0, 0, p, 1, p, 4, p, 16, 0, p, 1, p, 4, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_coverage(None, p, 4, 4, 1.0, 0, 0, 0, 0, 0, 16, p, 4, p, 16, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert lib.infur_frame_coverage_dev(None, p, 4, 4, 1.0, 0, 0, 0, 0, 0, 16, p, 4, p, 16, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


def test_the_command_line_wants_a_tolerance_with_shared_borders():
    with pytest.raises(SystemExit):
        segments_cli.main(["--width", "8", "--height", "8", "--synthetic-weights", "--outlines-out", os.devnull, "--outlines-shared"])


# ---------------------------------------------------------------- the reference against hand-written answers
def test_reference_on_a_hand_written_tee():
    # a bar of 1 over regions 2 (two wide) and 3 (one wide).  Lattice 4 x 4; (2, 1), id 6, is the T-junction: a corner of 2 and of 3
    # and a point inside the bar's lower edge 7 -> 4
    k = np.array([[1, 1, 1], [2, 2, 3], [2, 2, 3]], np.uint8)
    assert V.degrees(k).tolist() == [[2, 2, 2, 2], [3, 2, 3, 3], [2, 0, 2, 2], [2, 2, 3, 2]]
    l, v, c = O.outline(k)
    assert v.tolist() == [0, 3, 7, 4, 4, 6, 14, 12, 6, 7, 15, 14]
    lo, vo, co = V.coverage(k, l, v, c, 0)
    assert vo.tolist() == [0, 3, 7, 6, 4, 4, 6, 14, 12, 6, 7, 15, 14] and lo[:, :2].tolist() == [[0, 5], [5, 4], [9, 4]]
    assert co.tolist() == [3, 13, 0, 0, 13, 9]  # arcs: the bar 7..6, 6..4, 4..7 (round the corners 0, 3); region 2 and region 3 three each
    # one pixel: a plane corner is 0.707 px (2 x 2 region 3: 0.894 px at most) off the chord of its arc and goes; v_0 = 0 is dropped
    lo, vo, co = V.coverage(k, l, v, c, 16)
    assert vo.tolist() == [7, 6, 4, 4, 6, 14, 12, 6, 7, 14] and co.tolist() == [3, 10, 0, 0, 13, 9]
    # every border is there twice, once in each direction, except the frame 4 -> 7 -> 14 -> 12 (-> 4)
    assert V.frame_cycle(lo, vo) == [4, 7, 14, 12]
    assert set(V.segments(lo, vo)) >= {(7, 6), (6, 7), (6, 4), (4, 6), (6, 14), (14, 6)}
    # the same plane with region 3 skipped: none is a value of its own, the junction stays
    l, v, c = O.outline(k, O.SKIP, 3)
    lo, vo, co = V.coverage(k, l, v, c, 12, V.SKIP, 3)
    assert vo.tolist() == [0, 3, 6, 4, 4, 6, 14, 12] and co.tolist() == [2, 8, 0, 0, 9, 4]


def test_reference_status_words():
    k = np.array([[1, 1, 1], [2, 2, 3], [2, 2, 3]], np.uint8)
    l, v, c = O.outline(k)
    assert V.coverage(k, l, v, c, 16, loops_rows_in=2)[2].tolist() == [3, 0, 0, 1, 0, 0]
    assert V.coverage(k, l, v, c, 16, vertex_rows_in=11)[2].tolist() == [3, 0, 0, 1, 0, 0]
    assert V.coverage(k, l, v, c, 16, aug_rows=13)[2].tolist() == [3, 10, 0, 0, 13, 9]
    lo, vo, co = V.coverage(k, l, v, c, 16, aug_rows=12)
    assert co.tolist() == [3, 0, 0, 4, 13, 0] and len(lo) == 0 and len(vo) == 0
    bad = v.copy()
    bad[1] = 2 + 4  # (3, 0) -> (2, 1): two diagonal edges in loop 0
    lo, vo, co = V.coverage(k, l, bad, c, 16)
    assert co.tolist() == [3, 7, 1, 2, 8, 6] and lo[:, :2].tolist() == [[0, 0], [0, 4], [4, 3]] and vo.tolist() == [4, 6, 14, 12, 6, 7, 14]
    for ids in ([0, 0, 7, 4], [0, 3, 16, 4]):  # an edge of no length; an id outside the 4 x 4 lattice
        bad[:4] = ids
        assert V.coverage(k, l, bad, c, 16)[2].tolist() == co.tolist()
    short = l.copy()
    short[2, V.COUNT] = 1
    assert V.coverage(k, short, v, c, 16)[2][3] == 2
    short[2, V.COUNT] = 5  # ends beyond the vertices there are
    assert V.coverage(k, short, v, c, 16)[2][3] == 2


# ---------------------------------------------------------------- what the stage guarantees, on the planes of the GPU tests
@functools.lru_cache(maxsize=None)
def results(conn):
    out = []
    for name, k, skip, ringed in V.planes():
        l, v, c = O.outline(k, conn | (O.SKIP if skip is not None else 0), skip or 0)
        out.append([V.coverage(k, l, v, c, tol16, V.SKIP if skip is not None else 0, skip or 0) for tol16 in TOLS])
    return out


@pytest.mark.parametrize("conn", [0, CONN8])
def test_neighbours_fit_on_every_plane(conn):
    """N(p, q) = 0 except along one simple cycle, the frame; the shoelace sums agree; 2 h w on the ringed planes, whose frame is
    its four edges while the tolerance is below h w / sqrt(h^2 + w^2)"""
    ringed_seen = 0
    for (name, k, skip, ringed), per_tol in zip(V.planes(), results(conn)):
        for tol16, (lo, vo, co) in zip(TOLS, per_tol):
            assert co[3] == 0 and co[0] == len(lo) and co[1] == len(vo)
            if tol16 == 0:
                assert co[1] == co[4], name  # every augmented vertex is a corner or a junction: all are kept
            if skip is None:
                holds = ringed and V.ring_holds(k.shape, tol16)
                cycle = V.check_invariants(k, lo, vo, co, holds)
                ringed_seen += holds
                assert len(cycle) == 4 if holds else True, name
    assert ringed_seen >= 3 * 11  # the eleven ringed planes at 0, 11/16 and 12/16 px at least


def test_connectivity_does_not_change_what_is_kept():
    """the loops differ at every saddle; the junctions, the arcs and the kept vertices do not"""
    for (name, k, _, _), four, eight in zip(V.planes(), results(0), results(CONN8)):
        for (_, v4, c4), (_, v8, c8) in zip(four, eight):
            assert c4[[1, 4, 5]].tolist() == c8[[1, 4, 5]].tolist(), name
            assert sorted(v4.tolist()) == sorted(v8.tolist()), name
    assert any(len(a[0][0]) != len(b[0][0]) for a, b in zip(results(0), results(CONN8)))  # (there are saddles among the planes)


def test_simplify_alone_leaves_slivers():
    """what the stage is for: Douglas-Peucker loop by loop gives two neighbours two different chords"""
    k = R.smooth(135, 240, seed=750)
    l, v, c = O.outline(k)
    lo, vo, _ = S.simplify(l, v, c, 240, 16)
    seg = V.segments(lo, vo)
    lonely = sum(n for (p, q), n in seg.items() if (q, p) not in seg)
    assert lonely > sum(seg.values()) // 2  # most directed segments have no partner at all
    with pytest.raises(AssertionError):
        V.frame_cycle(lo, vo)
    lo, vo, co = V.coverage(k, l, v, c, 16)
    seg = V.segments(lo, vo)
    assert sum(n for (p, q), n in seg.items() if (q, p) not in seg) == len(V.frame_cycle(lo, vo))


PINNED = (
    (lambda: R.smooth(135, 240, seed=750), 5168, 218, {0: 5386, 11: 2958, 16: 1240, 64: 899}),
    (lambda: R.smooth(270, 480, seed=750), 21244, 854, {0: 22098, 12: 8410, 16: 4751, 32: 3650}),
    (lambda: R.noise(24, 40, 5, seed=3), 2618, 335, {0: 2953, 11: 2937, 16: 2723, 64: 2719}),
    (lambda: R.checkerboard(9, 11), 396, 0, {16: 392}),
)


@pytest.mark.parametrize("case", range(len(PINNED)))
def test_pinned_figures(case):
    """input vertices, inserted junctions and kept vertices as the stage was specified, the same under both connectivities"""
    make, n_vertices, inserted, kept = PINNED[case]
    k = make()
    for conn in (0, CONN8):
        l, v, c = O.outline(k, conn)
        assert c[1] == n_vertices
        for tol16, n in kept.items():
            lo, vo, co = V.coverage(k, l, v, c, tol16)
            assert co[1] == n and co[4] == n_vertices + inserted, (conn, tol16, co)
            V.check_invariants(k, lo, vo, co)
