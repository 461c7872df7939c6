"""Outlines (region boundaries as polygon loops) without a GPU: the ABI surface, the reference the GPU tests use
(tests/outlines_ref.py) against hand-written answers and its own invariants, and the helpers of infur_amd.processors."""
import ctypes as C
import os
import re
import sys

import numpy as np

from infur_amd import _lib
from infur_amd.processors import outlines_by_value, outlines_polygons

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_outlines", "infur_outlines_dev", "infur_frame_outlines", "infur_frame_outlines_dev")
CONSTANTS = {"INFUR_OUTLINES_SKIP": 1, "INFUR_OUTLINES_CONN8": 2, "INFUR_LOOP_OFFSET": 0, "INFUR_LOOP_COUNT": 1, "INFUR_LOOP_VALUE": 2,
             "INFUR_LOOP_START": 3, "INFUR_LOOP_WORDS": 4, "INFUR_FEATURE_OUTLINES": 16}
SKIP, CONN8 = O.SKIP, O.CONN8

RING = np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1],
                 [1, 0, 0, 0, 0, 0, 0, 0, 1],
                 [1, 0, 0, 0, 0, 0, 0, 0, 1],
                 [1, 0, 0, 1, 1, 0, 0, 0, 1],
                 [1, 0, 0, 0, 0, 0, 0, 0, 1],
                 [1, 0, 0, 0, 0, 0, 0, 0, 1],
                 [1, 1, 1, 1, 1, 1, 1, 1, 1]], np.uint8)
SADDLE = np.array([[1, 0], [0, 1]], np.uint8)


def planes():
    for h, w in ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (65, 130)):
        yield "smooth", R.smooth(h, w, seed=h)
        yield "noise2", R.noise(h, w, 2, seed=w)
        yield "noise21", R.noise(h, w, 21, seed=w)
        yield "single", R.single(h, w)
        yield "vstripes", R.stripes(h, w, vertical=True)
        yield "hstripes", R.stripes(h, w, vertical=False)
        yield "checkerboard", R.checkerboard(h, w)
        yield "staircase", R.staircase(h, w)
        yield "snake", O.snake(h, w)


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_OUTLINES
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    for older in (_lib.FEATURE_SEGMENTS, _lib.FEATURE_REGIONS, _lib.FEATURE_TRACKS, _lib.FEATURE_RUNS):  # the four older bits
        assert lib.infur_features() & older
    assert "pub struct HipOutlines" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Outlines" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def test_signatures_count_the_header_s_parameters():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    for s in NEW_SYMBOLS:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[s][1]), s


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert (O.SKIP, O.CONN8, O.OFFSET, O.COUNT, O.VALUE, O.START, O.WORDS) == (
        _lib.OUTLINES_SKIP, _lib.OUTLINES_CONN8, _lib.LOOP_OFFSET, _lib.LOOP_COUNT, _lib.LOOP_VALUE, _lib.LOOP_START, _lib.LOOP_WORDS)


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else and no output is touched"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_outlines(None, p, 1, 2, 2, 0, 0, 0, p, 4, p, 16, p) == _lib.E_INVALID_ARG
    assert lib.infur_outlines_dev(None, p, 4, 2, 2, 3, 9, 0, p, 4, p, 16, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_outlines(None, p, 4, 4, 1.0, 0, 0, 0, 0, 0, p, 4, p, 16, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert lib.infur_frame_outlines_dev(None, p, 4, 4, 1.0, 0, 0, 0, 0, 0, p, 4, p, 16, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


# ---------------------------------------------------------------- the reference against hand-written answers
def test_reference_on_the_ring_with_an_island():
    """7 x 9, class 0 skipped: the ring's outer boundary, the boundary of its hole (START & 3 == 2: the S side of pixel (7, 0), and
    it runs the other way round) and the island in the hole"""
    loops, vertices, counts = O.outline(RING, SKIP, 0)
    assert counts.tolist() == [3, 12, 62]
    assert loops.tolist() == [[0, 4, 1, 0], [4, 4, 1, 4 * 7 + 2], [8, 4, 1, 4 * (3 * 9 + 3)]]
    xy = [p[2] for p in O.polygons(loops, vertices, 9)]
    assert xy[0] == [(0, 0), (9, 0), (9, 7), (0, 7)]  # clockwise on a y-down screen; a rectangle is 4 vertices whatever its size
    assert xy[1] == [(8, 1), (1, 1), (1, 6), (8, 6)]  # counter-clockwise: the ring is on the right hand here too
    assert xy[2] == [(3, 3), (5, 3), (5, 4), (3, 4)]
    assert vertices.tolist() == [0, 9, 79, 70, 18, 11, 61, 68, 33, 35, 45, 43]
    assert [O.shoelace(p) for p in xy] == [126, -70, 4] and 126 - 70 + 4 == 2 * int((RING == 1).sum())
    O.check_invariants(RING, SKIP, 0, loops, vertices, counts)
    # nothing skipped: the background is a region too -- its outer boundary is the hole's, its hole the island's
    loops, vertices, counts = O.outline(RING)
    assert counts.tolist() == [5, 20, 62 + 24 + 6] and loops[:, O.VALUE].tolist() == [1, 1, 0, 0, 1] and (loops[:, O.START] & 3).tolist() == [0, 2, 0, 2, 0]
    O.check_invariants(RING, 0, 0, loops, vertices, counts)


def test_reference_on_the_saddle():
    loops, vertices, counts = O.outline(SADDLE, SKIP, 0)  # 4-connectivity: the two pixels are two regions
    assert counts.tolist() == [2, 8, 8] and loops.tolist() == [[0, 4, 1, 0], [4, 4, 1, 12]] and vertices.tolist() == [0, 1, 4, 3, 4, 5, 8, 7]
    loops, vertices, counts = O.outline(SADDLE, SKIP | CONN8, 0)  # 8-connectivity: one loop that passes vertex (1, 1) = 4 twice
    assert counts.tolist() == [1, 8, 8] and loops.tolist() == [[0, 8, 1, 0]] and vertices.tolist() == [0, 1, 4, 5, 8, 7, 4, 3]
    O.check_invariants(SADDLE, SKIP | CONN8, 0, loops, vertices, counts)
    # without skip the zeros are a region with the mirrored saddle
    assert O.outline(SADDLE, 0)[2].tolist() == [4, 16, 16] and O.outline(SADDLE, CONN8)[2].tolist() == [2, 16, 16]


def test_reference_on_one_pixel_capacity_and_empty_planes():
    loops, vertices, counts = O.outline(np.array([[5]], np.uint8))
    assert counts.tolist() == [1, 4, 4] and loops.tolist() == [[0, 4, 5, 0]] and vertices.tolist() == [0, 1, 3, 2]
    loops, vertices, counts = O.outline(np.array([[0xFFFFFFFF]], np.uint32))
    assert loops.tolist() == [[0, 4, 0xFFFFFFFF, 0]]
    assert O.outline(np.array([[5]], np.uint8), SKIP, 5)[2].tolist() == [0, 0, 0]  # everything skipped
    # max_edges one below n_edges: the edge count alone; exactly n_edges: the whole result
    loops, vertices, counts = O.outline(RING, SKIP, 0, max_edges=61)
    assert counts.tolist() == [0, 0, 62] and loops.shape == (0, 4) and vertices.shape == (0,)
    assert O.outline(RING, SKIP, 0, max_edges=62)[2].tolist() == [3, 12, 62]
    for h, w in ((0, 4), (3, 0), (0, 0)):
        loops, vertices, counts = O.outline(np.zeros((h, w), np.uint8))
        assert counts.tolist() == [0, 0, 0] and loops.shape == (0, 4) and vertices.shape == (0,)


def test_reference_invariants_on_the_families():
    counts = {}
    for name, k in planes():
        h, w = k.shape
        for plane in (k, U.as_u32(k)):
            for conn in (0, CONN8):
                res = O.outline(plane, conn)
                O.check_invariants(plane, conn, 0, *res)
                O.check_invariants_fast(plane, conn, 0, *res)
                counts[(name, h, w, conn)] = res[2].tolist()
                for skip in sorted({int(plane[0, 0]), int(plane[-1, -1])}):
                    sres = O.outline(plane, conn | SKIP, skip)
                    O.check_invariants(plane, conn | SKIP, skip, *sres)
                    # skipping takes loops of that value away and changes no other loop's vertices under 4-connectivity
                    assert sres[2][2] == int(O.edge_flags(plane, SKIP, skip).sum()) <= res[2][2]
    assert counts[("single", 65, 130, 0)] == [1, 4, 390] and counts[("checkerboard", 65, 130, 0)] == [8450, 33800, 33800]
    assert counts[("snake", 65, 130, 0)][0] == 33 and counts[("vstripes", 65, 130, 0)][1] == 4 * counts[("vstripes", 65, 130, 0)][0]


def test_reference_on_a_label_plane_starts_at_the_regions_first_pixels():
    k = R.smooth(65, 130)
    for connectivity in (4, 8):
        labels, table, n = R.label(k, None, connectivity, 6, R.SKIP_BACKGROUND)
        flags = SKIP | (CONN8 if connectivity == 8 else 0)
        res = O.outline(labels, flags, 0xFFFFFFFF)
        O.check_invariants(labels, flags, 0xFFFFFFFF, *res, first_of_label={i: int(table[i, R.FIRST]) for i in range(n)})


# ---------------------------------------------------------------- the helpers of the package
def test_helpers_of_the_package():
    loops, vertices, counts = O.outline(RING, SKIP, 0)
    polys = outlines_polygons(loops, vertices, 9)
    assert [(v, hole) for v, hole, _ in polys] == [(1, False), (1, True), (1, False)]
    assert all(xy.dtype == np.int32 and xy.shape == (4, 2) for _, _, xy in polys)
    assert [xy.tolist() for _, _, xy in polys] == [[list(p) for p in q[2]] for q in O.polygons(loops, vertices, 9)]
    by = outlines_by_value(loops, vertices, 9)
    assert sorted(by) == [1] and len(by[1]) == 2  # the ring with its hole, the island without one
    assert by[1][0][0].tolist() == [[0, 0], [9, 0], [9, 7], [0, 7]] and [h.tolist() for h in by[1][0][1]] == [[[8, 1], [1, 1], [1, 6], [8, 6]]]
    assert by[1][1][0].tolist() == [[3, 3], [5, 3], [5, 4], [3, 4]] and by[1][1][1] == []
    # truncated vertices: the loops whose vertices are all there
    assert len(outlines_polygons(loops, vertices[:7], 9)) == 1 and outlines_polygons(loops[:0], vertices, 9) == [] and outlines_by_value(loops[:0], vertices, 9) == {}
    for name, k in planes():
        if k.shape[0] * k.shape[1] > 2100:
            continue
        for plane in (k, U.as_u32(k)):
            res = O.outline(plane, CONN8)
            got, want = outlines_polygons(res[0], res[1], plane.shape[1]), O.polygons(res[0], res[1], plane.shape[1])
            assert len(got) == len(want) and all(g[0] == r[0] and g[1] == r[1] and g[2].tolist() == [list(p) for p in r[2]] for g, r in zip(got, want))
            by = outlines_by_value(res[0], res[1], plane.shape[1])
            assert sorted(by) == np.unique(plane).tolist() and sum(len(g) + sum(len(p[1]) for p in g) for g in by.values()) == len(want)


def test_rate_script_tables_without_a_device(capsys):
    """scripts/outlines_rate.py imports, generates its planes and formats both tables (made-up times: only the code path is checked)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("outlines_rate", os.path.join(ROOT, "scripts", "outlines_rate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dry-run"])
    lines = capsys.readouterr().out.splitlines()
    # smooth, one class, noise for u8 and u32, and the smooth plane again with max_edges = 1 Mi
    assert sum(line.startswith("| smooth") or line.startswith("| one class") or line.startswith("| noise") for line in lines) == 7
    assert sum("1048576" in line for line in lines if line.startswith("| smooth")) == 1
    assert sum(line.startswith("| f32 r50") for line in lines) == 3 and all(line.count("|") >= 7 for line in lines if line.startswith("|"))
    klass = R.smooth(54, 96)
    n_loops, n_vertices, n_edges = O.outline(klass)[2].tolist()
    assert f"| smooth 54x96 | u8 class | 0 | {n_edges} | {n_loops} | {n_vertices} |" in "\n".join(lines)
