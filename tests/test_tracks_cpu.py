"""Tracks (region identities carried from frame to frame) without a GPU: the ABI surface, the reference the GPU tests use
(tests/tracks_ref.py) against hand-written answers, and ``track_summary``."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import tracks_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_tracker_create", "infur_tracker_destroy", "infur_tracker_reset", "infur_tracks", "infur_tracks_dev", "infur_frame_tracks",
               "infur_frame_tracks_dev")
CONSTANTS = {"INFUR_TRACK_ID": 0, "INFUR_TRACK_AGE": 1, "INFUR_TRACK_BORN": 2, "INFUR_TRACK_PREV_REGION": 3, "INFUR_TRACK_OVERLAP": 4,
             "INFUR_TRACK_PREV_PIXELS": 5, "INFUR_TRACK_PREV_SUM_X": 6, "INFUR_TRACK_PREV_SUM_Y": 7, "INFUR_TRACK_WORDS": 8,
             "INFUR_TRACKS_TRUNCATED": 1, "INFUR_TRACKS_OVERFLOW": 2, "INFUR_TRACKS_IDS_EXHAUSTED": 4, "INFUR_TRACKS_SUMMARY_STATUS": 0,
             "INFUR_TRACKS_SUMMARY_CONTINUED": 1, "INFUR_TRACKS_SUMMARY_NEW": 2, "INFUR_TRACKS_SUMMARY_ENDED": 3,
             "INFUR_TRACKS_SUMMARY_WORDS": 4, "INFUR_FEATURE_TRACKS": 4}
NONE = T.NONE


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
    assert lib.infur_features() & _lib.FEATURE_TRACKS
    assert lib.infur_features() & _lib.FEATURE_REGIONS and lib.infur_features() & _lib.FEATURE_SEGMENTS
    assert "pub struct HipTracks" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Tracks" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert re.search(r"#define\s+INFUR_TRACK_NONE\s+0xFFFFFFFFu", header)
    assert re.search(r"pub const INFUR_TRACK_NONE\s*:\s*u32\s*=\s*0xFFFF_FFFF\s*;", rust)
    assert _lib.TRACK_NONE == 0xFFFFFFFF == NONE
    assert (T.ID, T.AGE, T.BORN, T.PREV_REGION, T.OVERLAP, T.PREV_PIXELS, T.PREV_SUM_X, T.PREV_SUM_Y, T.WORDS) == tuple(range(9))
    assert (T.TRUNCATED, T.OVERFLOW, T.IDS_EXHAUSTED) == (_lib.TRACKS_TRUNCATED, _lib.TRACKS_OVERFLOW, _lib.TRACKS_IDS_EXHAUSTED)
    assert (T.STATUS, T.CONTINUED, T.NEW, T.ENDED) == (0, 1, 2, 3)
    assert (T.DEFAULT_REGIONS, T.DEFAULT_SLOTS) == (65536, 1 << 20)


def test_argument_errors_need_no_gpu(lib):
    """a null tracker (or context) is refused before anything else and no output is touched"""
    ow, oh, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(77)
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    trk = C.c_void_p(0x1234)
    assert lib.infur_tracker_create(None, 0, 0, C.byref(trk)) == _lib.E_INVALID_ARG and trk.value == 0x1234
    assert lib.infur_tracker_reset(None, 5) == _lib.E_INVALID_ARG
    lib.infur_tracker_destroy(None)  # like free(NULL)
    assert lib.infur_tracks(None, p, p, 1, 1, 2, 2, 1, p, p, p, p) == _lib.E_INVALID_ARG
    assert lib.infur_tracks_dev(None, p, p, 1, p, 2, 2, 1, p, p, p, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_tracks(None, p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, None, 0, None, 0, C.addressof(n), None, C.byref(ow),
                                  C.byref(oh), None, 1, p, p, p, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_tracks_dev(None, p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, None, 0, None, 0, None, None, C.byref(ow),
                                      C.byref(oh), None, 1, p, p, p, p) == _lib.E_INVALID_ARG
    assert n.value == 77 and (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


# ---------------------------------------------------------------- the reference against hand-written answers
def steps(frames, **kw):
    return [s for _, _, _, s in T.run([np.array(f, np.uint8) for f in frames], **kw)]


def test_identical_frames_age_and_keep_their_ids():
    k = [[0, 0, 1, 1, 0, 2], [0, 0, 1, 1, 0, 2]]  # regions in first-pixel order: 0 (left), 1 (class 1), 0 (middle), 2
    a, b, c = steps([k, k, k])
    for i, s in enumerate((a, b, c)):
        assert s.track_of_region.tolist() == [0, 1, 2, 3]  # ids stable
        assert s.table[:, T.AGE].tolist() == [i + 1] * 4  # ages 1, 2, 3
        assert s.table[:, T.BORN].tolist() == [0] * 4
        assert s.plane.tolist() == [[0, 0, 1, 1, 2, 3]] * 2
    assert a.summary.tolist() == [0, 0, 4, 0] and b.summary.tolist() == [0, 4, 0, 0] == c.summary.tolist()
    assert a.table[:, T.PREV_REGION].tolist() == [NONE] * 4 and (a.table[:, T.OVERLAP:] == 0).all()
    assert b.table[1].tolist() == [1, 2, 0, 1, 4, 4, 2 + 3 + 2 + 3, 0 + 0 + 1 + 1]  # id, age, born, prev, overlap, pixels, sum x, sum y
    assert a.runs == 0 and b.runs == 8  # four runs per row


def test_a_moving_object_keeps_its_id_and_reports_its_step():
    f0 = np.zeros((5, 9), np.uint8)
    f0[1:3, 1:4] = 7
    f1 = np.roll(f0, (1, 2), axis=(0, 1))
    a, b = steps([f0, f1])
    assert b.track_of_region.tolist() == [0, 1] and b.table[1, T.AGE] == 2
    assert b.table[1, T.OVERLAP] == 1  # the 2 x 3 box moved by (1, 2): one pixel in common
    labels, table, n = T.regions_of(f1)
    dx = int(table[1, R.SUM_X]) / 6 - int(b.table[1, T.PREV_SUM_X]) / int(b.table[1, T.PREV_PIXELS])
    dy = int(table[1, R.SUM_Y]) / 6 - int(b.table[1, T.PREV_SUM_Y]) / int(b.table[1, T.PREV_PIXELS])
    assert (dx, dy) == (2.0, 1.0)
    # min_overlap above the common pixel: a new track, the old one ends
    a, b = steps([f0, f1], min_overlap=2)
    assert b.track_of_region.tolist() == [0, 2] and b.summary.tolist() == [0, 1, 1, 1]


def test_split_keeps_the_id_on_the_larger_part():
    whole, cut = T.split(8, 16)
    assert whole[2].tolist() == [0] + [1] * 14 + [0] and cut[2].tolist() == [0] + [1] * 4 + [2] + [1] * 9 + [0]
    a, b = steps([whole, cut])
    # frame 1 in first-pixel order: background, left part (4 wide), the cutting column, right part (9 wide)
    assert a.track_of_region.tolist() == [0, 1]
    assert b.track_of_region.tolist() == [0, 2, 3, 1]
    assert b.table[:, T.AGE].tolist() == [2, 1, 1, 2] and b.table[3, T.OVERLAP] == 2 * 9 and b.table[3, T.PREV_REGION] == 1
    assert b.table[:, T.BORN].tolist() == [0, 1, 1, 0]
    assert b.summary.tolist() == [0, 2, 2, 0]  # the loser did not fall back to a second choice: it is new


def test_merge_keeps_the_id_of_the_larger_contributor():
    cut, whole = T.merge(8, 16)
    a, b = steps([cut, whole])
    assert a.track_of_region.tolist() == [0, 1, 2, 3]
    assert b.track_of_region.tolist() == [0, 3] and b.table[1].tolist()[:5] == [3, 2, 0, 3, 18]
    assert b.summary.tolist() == [0, 2, 0, 2]  # the smaller part and the column ended


def test_equal_halves_exercise_both_tie_rules():
    whole, cut = T.split(8, 17, equal=True)
    assert cut[2].tolist() == [0] + [1] * 7 + [2] + [1] * 7 + [0]
    a, b = steps([whole, cut])
    # both halves choose the bar with overlap 14; the bar is kept by the smaller region id: the left half
    assert b.track_of_region.tolist() == [0, 1, 2, 3] and b.table[:, T.AGE].tolist() == [2, 2, 1, 1]
    a, b = steps([cut, whole])
    # the bar overlaps both halves by 14 pixels; it chooses the smaller remembered id: the left half's track
    assert a.track_of_region.tolist() == [0, 1, 2, 3]
    assert b.track_of_region.tolist() == [0, 1] and b.table[1, T.PREV_REGION] == 1 and b.table[1, T.OVERLAP] == 14


def test_class_change_starts_a_new_track():
    a, b, c = steps(T.class_change(8, 16))
    assert a.track_of_region.tolist() == [0, 1] and b.track_of_region.tolist() == [0, 2] and c.track_of_region.tolist() == [0, 2]
    assert b.summary.tolist() == [0, 1, 1, 1] and c.table[:, T.AGE].tolist() == [3, 2] and c.table[1, T.BORN] == 1


def test_an_object_absent_for_a_frame_returns_with_a_new_id():
    a, b, c = steps(T.gap(8, 16))
    assert a.track_of_region.tolist() == [0, 1] and b.track_of_region.tolist() == [0] and c.track_of_region.tolist() == [0, 2]
    assert b.summary.tolist() == [0, 1, 0, 1] and c.summary.tolist() == [0, 1, 1, 0]
    assert c.table[:, T.AGE].tolist() == [3, 1] and c.table[:, T.BORN].tolist() == [0, 2]


def test_truncation_reset_resize_overflow_and_exhaustion():
    k = np.array([[0, 1, 0, 2, 0, 3]], np.uint8)  # six regions
    labels, table, n = T.regions_of(k)
    # max_regions below n: the first three are tracked
    t = T.Tracker(max_regions=3)
    s = t.step(labels, table, n)
    assert s.track_of_region.tolist() == [0, 1, 2, NONE, NONE, NONE] and s.summary.tolist() == [T.TRUNCATED, 0, 3, 0]
    assert s.plane.tolist() == [[0, 1, 2, NONE, NONE, NONE]] and s.table[3].tolist() == [NONE, 0, 0, NONE, 0, 0, 0, 0]
    s = t.step(labels, table, n)
    assert s.track_of_region.tolist() == [0, 1, 2, NONE, NONE, NONE] and s.summary.tolist() == [T.TRUNCATED, 3, 0, 0]
    # table_rows below n: only those rows exist
    t = T.Tracker()
    s = t.step(labels, table[:2], n)
    assert s.track_of_region.tolist() == [0, 1] and s.summary[T.STATUS] == T.TRUNCATED and len(s.table) == 2
    # reset: everything new from the given id; another shape: everything new, ids keep counting
    t.reset(100)
    s = t.step(labels, table, n)
    assert s.track_of_region.tolist() == list(range(100, 106)) and s.summary.tolist() == [0, 0, 6, 0]
    assert s.table[:, T.BORN].tolist() == [1] * 6  # the frame counter is the tracker's, not the reset's
    l2, t2, n2 = T.regions_of(k.reshape(2, 3))
    s = t.step(l2, t2, n2)
    assert s.track_of_region.tolist() == list(range(106, 106 + n2)) and s.summary.tolist() == [0, 0, n2, 0]
    # an empty frame forgets
    s = t.step(np.zeros((0, 3), np.uint32), np.zeros((0, 10), np.uint64), 0)
    assert s.summary.tolist() == [0, 0, 0, 0]
    assert t.step(l2, t2, n2).summary.tolist() == [0, 0, n2, 0]
    # exhaustion: 0xFFFFFFF0 + 6 fits, the next six do not
    t = T.Tracker()
    t.reset(0xFFFFFFF0)
    assert t.step(labels, table, n).track_of_region.tolist() == list(range(0xFFFFFFF0, 0xFFFFFFF6))
    t.reset(0xFFFFFFFA)
    s = t.step(labels, table, n)
    assert s.track_of_region.tolist() == [NONE] * 6 and s.summary.tolist() == [T.IDS_EXHAUSTED, 0, 0, 0] and t.next_id == 0xFFFFFFFA
    assert (s.plane == NONE).all()
    # overflow: 65 x 130 noise has thousands of runs; a 64-slot table reports it, remembers the frame and tracks the next one
    t = T.Tracker(pair_slots=64)
    f = [T.regions_of(x) for x in (R.noise(65, 130, 3, 0), R.noise(65, 130, 3, 1))]
    a, b = t.step(*f[0]), t.step(*f[1])
    assert a.summary[T.STATUS] == 0 and b.summary[T.STATUS] == T.OVERFLOW and 2 * b.runs > 64
    assert b.summary.tolist() == [T.OVERFLOW, 0, f[1][2], f[0][2]] and b.track_of_region.tolist() == list(range(f[0][2], f[0][2] + f[1][2]))
    small = T.regions_of(R.single(2, 64))
    t = T.Tracker(pair_slots=64)
    assert [t.step(*small).summary.tolist() for _ in range(2)] == [[0, 0, 1, 0], [0, 1, 0, 0]]


def test_no_default_slot_case_overflows():
    """the largest plane of the GPU tests has 129,600 pixels, hence at most as many runs, against a threshold of 524,288"""
    for name in ("cross", "noise3"):
        for _, _, _, s in T.run(T.FAMILIES[name](65, 130)):
            assert 2 * s.runs <= T.DEFAULT_SLOTS and not s.summary[T.STATUS] & T.OVERFLOW
    assert 2 * 270 * 480 <= T.DEFAULT_SLOTS


def test_track_summary_records():
    from infur_amd.processors import track_summary

    f0 = np.zeros((5, 9), np.uint8)
    f0[1:3, 1:4] = 15
    f1 = np.roll(f0, (1, 2), axis=(0, 1))
    f1[0, 8] = 3
    (_, _, _, a), (labels, table, n, b) = T.run([f0, f1])
    recs = track_summary(table, b.table, n, 9, 5)
    assert [r["track"] for r in recs] == [0, 2, 1] and [r["age"] for r in recs] == [2, 1, 2] and [r["name"] for r in recs][2] == "person"
    assert recs[2]["step"] == (2.0, 1.0) and recs[2]["prev_region"] == 1 and recs[2]["overlap"] == 1 and recs[2]["box"] == (3, 2, 5, 3)
    assert recs[1]["step"] is None and recs[1]["prev_region"] is None and recs[1]["born"] == 1
    untracked = b.table.copy()
    untracked[1] = [NONE, 0, 0, NONE, 0, 0, 0, 0]
    assert track_summary(table, untracked, n, 9, 5)[1]["track"] is None
    assert len(track_summary(table, b.table[:2], n, 9, 5)) == 2 and track_summary(table[:0], b.table[:0], 0, 9, 5) == []


def test_tracks_processor_validates_commands_without_a_gpu():
    from infur_amd.processors import InfurError, Tracks, TracksCmd

    t = Tracks.__new__(Tracks)  # (no context here: the tracker itself is made on the device)
    t.ctx, t.t, t.min_overlap, t.dirty = None, None, 1, False
    for bad in (TracksCmd(), TracksCmd(min_overlap=1, reset=0), TracksCmd.MinOverlap(-1), TracksCmd.MinOverlap(1 << 32)):
        with pytest.raises(InfurError):
            t.control(bad)
    assert not t.is_dirty() and t.min_overlap == 1
    assert not t.control(TracksCmd.MinOverlap(1)).is_dirty()
    assert t.control(TracksCmd.MinOverlap(9)).is_dirty() and t.min_overlap == 9
