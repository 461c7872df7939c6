"""Regions (connected components of the class plane) without a GPU: the ABI surface, the two implementations of the reference
the GPU tests use (tests/regions_ref.py) against each other and against hand-written answers, the identity that ties the region
table to Segments' per-class statistics, and ``region_summary``."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import segments_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_regions", "infur_regions_dev", "infur_frame_regions", "infur_frame_regions_dev")
CONSTANTS = {"INFUR_CONNECT_4": 4, "INFUR_CONNECT_8": 8, "INFUR_REGIONS_SKIP_BACKGROUND": 1, "INFUR_REGION_CLASS": 8,
             "INFUR_REGION_FIRST": 9, "INFUR_REGION_WORDS": 10, "INFUR_FEATURE_REGIONS": 2}
NONE = int(R.NONE)


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    assert lib.infur_features() & _lib.FEATURE_REGIONS
    assert lib.infur_features() & _lib.FEATURE_SEGMENTS
    assert "pub struct HipRegions" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert re.search(r"#define\s+INFUR_REGION_NONE\s+0xFFFFFFFFu", header)
    assert re.search(r"pub const INFUR_REGION_NONE\s*:\s*u32\s*=\s*0xFFFF_FFFF\s*;", rust)
    assert _lib.REGION_NONE == 0xFFFFFFFF == NONE
    assert (R.CONNECT_4, R.CONNECT_8, R.SKIP_BACKGROUND, R.CLASS, R.FIRST, R.WORDS) == (4, 8, 1, 8, 9, 10)
    assert (R.PIXELS, R.MAX_Y) == (_lib.STAT_PIXELS, _lib.STAT_MAX_Y)


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else, like every other entry point"""
    ow, oh, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(77)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_regions(None, p, None, 4, 4, 4, 0, 0, None, None, 0, C.addressof(n)) == _lib.E_INVALID_ARG
    assert lib.infur_regions_dev(None, None, None, 4, 4, 8, 0, 0, None, None, 0, None) == _lib.E_INVALID_ARG
    assert lib.infur_frame_regions(None, p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, None, 0, None, 0, C.addressof(n), None, C.byref(ow),
                                   C.byref(oh)) == _lib.E_INVALID_ARG
    assert lib.infur_frame_regions_dev(None, p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, None, 0, None, 0, None, None, C.byref(ow),
                                       C.byref(oh)) == _lib.E_INVALID_ARG
    assert n.value == 77


# ---------------------------------------------------------------- the two reference implementations
def families():
    yield "smooth 33x47", R.smooth(33, 47)
    yield "smooth 270x480", R.smooth(270, 480)
    yield "noise21 270x480", R.noise(270, 480, 21)
    yield "noise3 65x130", R.noise(65, 130, 3)
    yield "single 65x130", R.single(65, 130)
    yield "serpentine 65x130", R.serpentine(65, 130)
    yield "spiral 65x130", R.spiral(65, 130, arms=2)
    yield "vstripes 33x47", R.stripes(33, 47, vertical=True)
    yield "hstripes 33x47", R.stripes(33, 47, vertical=False)
    yield "staircase 65x130", R.staircase(65, 130)
    yield "checkerboard 33x47", R.checkerboard(33, 47)
    for h, w in ((1, 1), (1, 300), (300, 1), (3, 5)):
        yield f"noise3 {h}x{w}", R.noise(h, w, 3, seed=h + w)


@pytest.mark.skipif(not R.HAVE_SCIPY, reason="scipy is not installed: the numpy implementation stands alone")
def test_the_two_reference_implementations_agree():
    for name, k in families():
        cf = R.conf_for(k)
        for conn in (4, 8):
            for min_pixels, flags in ((0, 0), (3, R.SKIP_BACKGROUND)):
                a = R.label(k, cf, conn, min_pixels, flags, impl="scipy")
                b = R.label(k, cf, conn, min_pixels, flags, impl="numpy")
                assert a[2] == b[2], (name, conn, min_pixels, flags)
                assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), (name, conn, min_pixels, flags)


IMPLS = ["numpy"] + (["scipy"] if R.HAVE_SCIPY else [])


@pytest.mark.parametrize("impl", IMPLS)
def test_known_answers(impl):
    lab = lambda k, conn, **kw: R.label(np.array(k, np.uint8), kw.pop("conf", None), conn, impl=impl, **kw)  # noqa: E731
    # 3 x 3 checkerboard: nine regions at connectivity 4, two at connectivity 8
    cb = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    labels, table, n = lab(cb, 4)
    assert n == 9 and labels.ravel().tolist() == list(range(9))
    assert table[:, R.FIRST].tolist() == list(range(9)) and table[:, R.CLASS].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert (table[:, R.PIXELS] == 1).all() and table[:, R.SUM_X].tolist() == [0, 1, 2] * 3 and table[:, R.MAX_Y].tolist() == [0] * 3 + [1] * 3 + [2] * 3
    labels, table, n = lab(cb, 8)
    assert n == 2 and labels.tolist() == cb
    assert table.tolist() == [[5, 5, 5, 0, 0, 0, 2, 2, 0, 0], [4, 4, 4, 0, 0, 0, 2, 2, 1, 1]]
    # a two-arm spiral: two regions under either connectivity, however many turns
    for h, w in ((9, 11), (40, 70)):
        sp = R.spiral(h, w, arms=2)
        for conn in (4, 8):
            labels, table, n = lab(sp, conn)
            assert n == 2 and (labels == (sp == 2)).all(), (h, w, conn)
            assert table[0, R.CLASS] == 1 and table[1, R.CLASS] == 2 and table[1, R.FIRST] == w
            assert table[0, R.PIXELS] + table[1, R.PIXELS] == h * w
    # a "U" whose arms join only in the last row: one region although the arms' provisional labels differ
    u = np.zeros((6, 5), np.uint8)
    u[:, 0] = u[:, 4] = u[5, :] = 4
    labels, table, n = lab(u, 4)
    assert n == 2 and labels[0, 0] == 0 and labels[0, 4] == 0 and labels[0, 1] == 1
    assert table[0].tolist() == [15, 6 * 0 + 6 * 4 + 1 + 2 + 3, 2 * 15 + 3 * 5, 0, 0, 0, 4, 5, 4, 0]
    assert table[1].tolist() == [15, 5 * 6, 3 * 10, 0, 1, 0, 3, 4, 0, 1]
    # one class over the whole plane
    labels, table, n = lab(np.full((7, 9), 6), 8, conf=np.full((7, 9), 200, np.uint8))
    assert n == 1 and (labels == 0).all() and table[0].tolist() == [63, 7 * 36, 9 * 21, 63 * 200, 0, 0, 8, 6, 6, 0]
    # min_pixels and skip-background: rows of 0 0 1 1 1 0 2 0 -- a triple of class 1, a single pixel of class 2, three background pieces
    row = [[0, 0, 1, 1, 1, 0, 2, 0]]
    labels, table, n = lab(row, 4)
    assert n == 5 and labels.tolist() == [[0, 0, 1, 1, 1, 2, 3, 4]]
    for mp in (0, 1):
        assert lab(row, 4, min_pixels=mp)[2] == 5  # 0 and 1 keep everything
    labels, table, n = lab(row, 4, min_pixels=2)
    assert n == 2 and labels.tolist() == [[0, 0, 1, 1, 1, NONE, NONE, NONE]] and table[:, R.PIXELS].tolist() == [2, 3]
    labels, table, n = lab(row, 4, flags=R.SKIP_BACKGROUND)
    assert n == 2 and labels.tolist() == [[NONE, NONE, 0, 0, 0, NONE, 1, NONE]] and table[:, R.CLASS].tolist() == [1, 2]
    labels, table, n = lab(row, 4, min_pixels=2, flags=R.SKIP_BACKGROUND)
    assert n == 1 and table[0].tolist() == [3, 9, 0, 0, 2, 0, 4, 0, 1, 2]
    labels, table, n = lab(row, 4, min_pixels=4)
    assert n == 0 and (labels == NONE).all() and table.shape == (0, 10)
    # an empty image
    labels, table, n = R.label(np.zeros((0, 5), np.uint8), None, 8, impl=impl)
    assert n == 0 and labels.shape == (0, 5) and table.shape == (0, 10)


def test_truncation_rule_is_a_prefix():
    """table_rows < n: the library writes the first table_rows rows of the same table and the full count; labels are complete"""
    k = R.noise(20, 30, 3)
    labels, table, n = R.label(k, R.conf_for(k), 4)
    assert n > 8 and (labels.max() == n - 1) and (table[:8, R.FIRST] < table[8, R.FIRST]).all()
    assert (np.diff(table[:, R.FIRST].astype(np.int64)) > 0).all()  # ascending FIRST: a prefix is well defined


@pytest.mark.parametrize("impl", IMPLS)
def test_region_rows_add_up_to_the_class_statistics(impl):
    """for every class, the sum / min / max of its region rows is Segments' row of that class (nothing dropped)"""
    for name, k in families():
        cf = R.conf_for(k, seed=3)
        st = S.stats(k, cf, 21)
        for conn in (4, 8):
            labels, table, n = R.label(k, cf, conn, impl=impl)
            assert (labels != NONE).all() and n == len(table)
            agg = np.zeros((21, 8), np.uint64)
            agg[:, [S.MIN_X, S.MIN_Y]] = S.U64_MAX
            for c in range(21):
                rows = table[table[:, R.CLASS] == c]
                if len(rows):
                    agg[c, :4] = rows[:, :4].sum(axis=0)
                    agg[c, 4:6] = rows[:, 4:6].min(axis=0)
                    agg[c, 6:8] = rows[:, 6:8].max(axis=0)
            assert (agg == st).all(), (name, conn)
            # ... and a row describes its own pixels
            firsts = table[:, R.FIRST].astype(np.int64)
            assert (labels.ravel()[firsts] == np.arange(n)).all() and (k.ravel()[firsts] == table[:, R.CLASS]).all()


def test_region_summary_records():
    from infur_amd.processors import region_summary

    kl = np.zeros((4, 6), np.uint8)
    kl[1:3, 0:2] = 15
    kl[1:3, 4:6] = 15
    cf = np.full((4, 6), 51, np.uint8)
    cf[kl == 15] = 255
    labels, table, n = R.label(kl, cf, 8)
    recs = region_summary(table, n, 6, 4)
    assert [r["name"] for r in recs] == ["__background__", "person", "person"] and [r["id"] for r in recs] == [0, 1, 2]
    left, right = recs[1], recs[2]
    assert left["pixels"] == 4 and left["share"] == 4 / 24 and left["box"] == (0, 1, 1, 2) and left["centroid"] == (0.5, 1.5)
    assert right["box"] == (4, 1, 5, 2) and right["centroid"] == (4.5, 1.5) and right["first"] == (4, 1) and right["klass"] == 15
    assert left["mean_confidence"] == 1.0 and abs(recs[0]["mean_confidence"] - 0.2) < 1e-12 and recs[0]["first"] == (0, 0)
    assert region_summary(table, n, 6, 4, names=["bg"])[1]["name"] == "class15"
    assert len(region_summary(table[:2], n, 6, 4)) == 2  # a truncated table: the rows there are
    assert region_summary(table[:0], 0, 6, 4) == []


def test_regions_processor_validates_commands_without_a_gpu():
    from infur_amd.processors import InfurError, Regions, RegionsCmd

    r = Regions(None)
    r.dirty = False
    for bad in (RegionsCmd.Connectivity(6), RegionsCmd.Flags(2), RegionsCmd(), RegionsCmd(connectivity=4, flags=0)):
        with pytest.raises(InfurError):
            r.control(bad)
    assert not r.is_dirty() and (r.connectivity, r.min_pixels, r.flags) == (8, 0, 0)  # state untouched
    assert not r.control(RegionsCmd.Connectivity(8)).is_dirty()
    assert r.control(RegionsCmd.MinPixels(16)).is_dirty() and r.min_pixels == 16
    assert r.control(RegionsCmd.Flags(_lib.REGIONS_SKIP_BACKGROUND)).flags == 1 and r.control(RegionsCmd.Connectivity(4)).connectivity == 4
