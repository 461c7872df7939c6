"""Tracks' memory (a gallery of lost tracks) without a GPU: the ABI surface, and the reference the GPU tests use
(tests/tracks_memory_ref.py) against hand-written answers and recorded numbers."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracks_memory_ref as M  # noqa: E402
import tracks_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_tracker_set_memory", "infur_tracker_memory", "infur_tracker_memory_dev")
CONSTANTS = {"INFUR_FEATURE_TRACK_MEMORY": 128, "INFUR_TRACKS_GALLERY_FULL": 8, "INFUR_LOST_ID": 0, "INFUR_LOST_AGE": 1, "INFUR_LOST_BORN": 2,
             "INFUR_LOST_CLASS": 3, "INFUR_LOST_PIXELS": 4, "INFUR_LOST_SUM_X": 5, "INFUR_LOST_SUM_Y": 6, "INFUR_LOST_MIN_X": 7, "INFUR_LOST_MIN_Y": 8,
             "INFUR_LOST_MAX_X": 9, "INFUR_LOST_MAX_Y": 10, "INFUR_LOST_SEEN": 11, "INFUR_LOST_WORDS": 12, "INFUR_TRACK_MEMORY_REVIVED": 0,
             "INFUR_TRACK_MEMORY_LOST": 1, "INFUR_TRACK_MEMORY_EXPIRED": 2, "INFUR_TRACK_MEMORY_HELD": 3, "INFUR_TRACK_MEMORY_WORDS": 4}


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
    assert lib.infur_features() & _lib.FEATURE_TRACK_MEMORY == 128
    assert lib.infur_features() & 127 == 127  # the seven older bits
    wrapper = open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "pub fn set_memory" in wrapper and "pub fn memory" in wrapper
    hpp = open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()
    assert "Status set_memory(" in hpp and "Status memory(" in hpp
    assert "There is no memory beyond one frame" not in header


def _args(text, start):
    """the top-level arguments of the call whose opening parenthesis is at text[start]"""
    depth, out, cur = 0, [], ""
    for ch in text[start:]:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if depth == 0:
            return out + [cur.strip()]
        if ch == "," and depth == 1:
            out, cur = out + [cur.strip()], ""
        elif depth > 1 or ch != "(":
            cur += ch
    raise AssertionError("unbalanced call")


def test_the_rust_wrapper_calls_match_the_declarations():
    """the wrapper crate is not compiled by this suite: at least every call of a memory function passes as many arguments as the
    sys crate declares, and every sys constant it names exists"""
    sys_rs = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    wrapper = open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    for s in ("infur_tracker_set_memory", "infur_tracker_memory"):
        decl = re.search(r"pub fn %s\s*\(" % s, sys_rs)
        call = re.search(r"sys::%s\s*\(" % s, wrapper)
        assert decl and call, s
        assert len(_args(wrapper, call.end() - 1)) == len(_args(sys_rs, decl.end() - 1)), s
    body = wrapper[wrapper.index("impl HipTracks {"):wrapper.index("impl Drop for HipTracks")]
    assert "pub fn set_memory" in body and "pub fn memory" in body and "pub struct TracksMemory" in body
    for name in set(re.findall(r"sys::(INFUR_[A-Z0-9_]+)", body)):
        assert re.search(r"pub const %s\s*:" % name, sys_rs), name
    assert body.count("{") == body.count("}") and body.count("(") == body.count(")")


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert (M.L_ID, M.L_AGE, M.L_BORN, M.L_CLASS, M.L_PIXELS, M.L_SUM_X, M.L_SUM_Y, M.L_MIN_X, M.L_MIN_Y, M.L_MAX_X, M.L_MAX_Y, M.L_SEEN,
            M.L_WORDS) == tuple(range(13))
    assert (M.REVIVED, M.LOST, M.EXPIRED, M.HELD) == (0, 1, 2, 3) and M.GALLERY_FULL == _lib.TRACKS_GALLERY_FULL
    assert (M.DEFAULT_ROWS, M.MAX_ROWS) == (4096, 65536)


def test_argument_errors_need_no_gpu(lib):
    """a null tracker is refused before anything else and no output is touched"""
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_tracker_set_memory(None, 1, 0, 0) == _lib.E_INVALID_ARG
    assert lib.infur_tracker_set_memory(None, 0, 0, 0) == _lib.E_INVALID_ARG
    assert lib.infur_tracker_memory(None, p, 2, p, p, 1) == _lib.E_INVALID_ARG
    assert lib.infur_tracker_memory_dev(None, p, 2, p, p, 1) == _lib.E_INVALID_ARG
    assert (buf == 0xA5).all()


# ---------------------------------------------------------------- the reference against hand-written answers
def steps(frames, **kw):
    return [s for _, _, _, s in M.run(frames, **kw)]


def summaries(ss):
    return [s.summary.tolist() for s in ss], [s.memory.tolist() for s in ss]


def test_gap_a_flicker_keeps_its_id():
    ss = steps(T.gap(65, 130), max_lost=1)
    assert summaries(ss) == ([[0, 0, 2, 0], [0, 1, 0, 1], [0, 1, 0, 0]], [[0, 0, 0, 0], [0, 1, 0, 1], [1, 0, 0, 0]])
    last = ss[-1]
    assert last.track_of_region.tolist() == [0, 1] and last.table[:, T.AGE].tolist() == [3, 2] and last.gap_of_region.tolist() == [0, 1]
    assert last.table[1, T.BORN] == 0 and last.table[1, T.PREV_REGION] == T.NONE and last.table[1, T.OVERLAP] == 0
    bar = ss[0].table  # the entry carried the bar's last region: its words return as PREV_*
    labels, table, n = T.regions_of(T.gap(65, 130)[0])
    assert last.table[1, T.PREV_PIXELS:].tolist() == [int(table[1, c]) for c in (0, 1, 2)] and bar[1, T.AGE] == 1
    e = ss[1].gallery
    assert e.shape == (1, 12) and e[0, :4].tolist() == [1, 1, 0, 1] and e[0, M.L_SEEN] == 0
    assert e[0, M.L_MIN_X:M.L_SEEN].tolist() == [1, 65 // 4, 128, 65 // 2 - 1] and len(last.gallery) == 0


def test_gap2_expires_after_max_lost():
    ss = steps(M.gap2(65, 130), max_lost=1)
    assert ss[2].memory.tolist() == [0, 0, 0, 1] and ss[3].memory.tolist() == [0, 0, 1, 0]
    assert ss[3].track_of_region.tolist() == [0, 2] and ss[3].summary.tolist() == [0, 1, 1, 0]
    ss = steps(M.gap2(65, 130), max_lost=2)
    assert ss[3].memory.tolist() == [1, 0, 0, 0] and ss[3].gap_of_region.tolist() == [0, 2] and ss[3].table[:, T.AGE].tolist() == [4, 2]


def test_one_row_both_outer_pieces():
    ss = steps(T.gap(1, 300), max_lost=1)
    assert ss[0].summary.tolist() == [0, 0, 3, 0] and ss[-1].memory.tolist() == [2, 0, 0, 0]
    assert ss[-1].track_of_region.tolist() == [0, 1, 2] and ss[-1].summary.tolist() == [0, 1, 0, 0]  # one continues, two are revived


def test_drift_needs_reach():
    for reach in (0, 4):
        ss = steps(M.drift(65, 130), max_lost=1, reach=reach)
        assert ss[-1].summary.tolist() == [0, 1, 1, 0] and ss[-1].memory[M.REVIVED] == 0
    ss = steps(M.drift(65, 130), max_lost=1, reach=65 // 2)
    assert ss[-1].memory.tolist() == [1, 0, 0, 0] and ss[-1].track_of_region.tolist() == [0, 1]
    # no reach can wrap: the product is clamped
    ss = steps(M.drift(65, 130), max_lost=1, reach=0xFFFFFFFF)
    assert ss[-1].memory.tolist() == [1, 0, 0, 0]


def test_the_five_tie_cases():
    last = lambda f, reach=16: steps(f(), max_lost=1, reach=reach)[-1]  # noqa: E731
    s = last(M.tie_two_to_one)  # both entries score 64: the smaller gallery index, the x = 8 square
    assert s.track_of_region.tolist() == [0, 1] and s.memory[M.HELD] == 1 and s.gallery[0, M.L_ID] == 2
    s = last(M.tie_two_to_one, 8)  # out of reach
    assert s.track_of_region.tolist() == [0, 3] and s.memory.tolist() == [0, 0, 0, 2]
    s = last(M.tie_one_to_two)  # both squares choose the entry with score 64: the smaller c
    assert s.track_of_region.tolist() == [0, 1, 2] and s.gap_of_region.tolist() == [0, 1, 0]
    s = last(M.tie_larger_score)  # the 12-wide block overlaps the grown box more
    assert s.track_of_region.tolist() == [0, 2, 1]
    s = last(M.tie_other_class)
    assert s.track_of_region.tolist() == [0, 2] and s.memory.tolist() == [0, 0, 0, 1]


def test_without_memory_it_is_tracks_ref():
    for name, family in T.FAMILIES.items():
        for (_, _, _, a), (_, _, _, b) in zip(T.run(family(65, 130)), M.run(family(65, 130))):
            assert (a.track_of_region == b.track_of_region).all() and (a.table == b.table).all() and (a.plane == b.plane).all(), name
            assert a.summary.tolist() == b.summary.tolist() and a.runs == b.runs and b.memory is None and b.gap_of_region is None, name


def test_flicker_numbers():
    ss = steps(M.flicker(270, 480), max_lost=1)
    assert ss[-1].summary.tolist() == [0, 493, 0, 23] and ss[-1].memory.tolist() == [26, 23, 0, 23]
    ss = steps(M.flicker(65, 130), max_lost=1)
    assert ss[-1].summary.tolist() == [0, 41, 0, 1] and ss[-1].memory.tolist() == [2, 1, 0, 1]
    for s in ss:
        assert s.summary[T.CONTINUED] + s.summary[T.NEW] + s.memory[M.REVIVED] == len(s.track_of_region)


def test_ragged_numbers():
    frames = M.ragged4(M.ragged_scan_frames())
    for rows in (0, 64):
        t = M.Tracker(max_lost=2, gallery_rows=rows)
        ss = [t.step(*f) for f in frames]
        mem = [s.memory.tolist() for s in ss]
        if rows == 0:
            assert mem[1:] == [[0, 1405, 0, 1405], [1374, 1357, 0, 1388], [1350, 1405, 0, 1443]] and all(s.summary[T.STATUS] == 0 for s in ss)
        else:
            assert [int(s.summary[T.STATUS]) for s in ss] == [0, 8, 8, 8] and [m[M.HELD] for m in mem[1:]] == [64, 64, 64]
            assert [m[M.REVIVED] for m in mem[2:]] == [64, 63]
            assert (ss[1].gallery[:, M.L_SEEN] == 0).all() and len(ss[1].gallery) == 64  # the last 64 of the 1405 lost: dropped from the front


def test_exhaustion_empties_the_gallery_and_reset_forgets():
    frames = [T.regions_of(k) for k in T.gap(8, 16)]
    t = M.Tracker(max_lost=1)
    t.reset(0xFFFFFFFC)
    a, b, c = [t.step(*f) for f in frames]
    assert c.summary.tolist() == [0, 1, 0, 0] and c.memory.tolist() == [1, 0, 0, 0]  # without memory this step exhausts the ids
    u = T.Tracker()
    u.reset(0xFFFFFFFC)
    assert [u.step(*f) for f in frames][-1].summary[T.STATUS] == T.IDS_EXHAUSTED
    t.step(*frames[1])
    assert len(t.gallery) == 1
    s = t.step(*T.regions_of(np.arange(128, dtype=np.uint8).reshape(8, 16) % 5))
    assert s.summary[T.STATUS] == T.IDS_EXHAUSTED and s.memory.tolist() == [0, 0, 0, 0] and len(s.gallery) == 0
    t = M.Tracker(max_lost=1)
    t.step(*frames[0]), t.step(*frames[1])
    t.reset(9)
    s = t.step(*frames[2])
    assert s.track_of_region.tolist() == [9, 10] and s.memory.tolist() == [0, 0, 0, 0]


def test_track_summary_adds_the_gap():
    from infur_amd.processors import track_summary

    (_, _, _, _), (_, _, _, _), (labels, table, n, s) = M.run(T.gap(8, 16), max_lost=1)
    recs = track_summary(table, s.table, n, 16, 8, gap=s.gap_of_region)
    assert [r["gap"] for r in recs] == [0, 1] and recs[1]["track"] == 1 and recs[1]["age"] == 2 and recs[1]["prev_region"] is None
    assert "gap" not in track_summary(table, s.table, n, 16, 8)[0]


def test_tracks_processor_without_memory_reports_none():
    from infur_amd.processors import Tracks, TracksOut

    t = Tracks.__new__(Tracks)  # (no context here: the tracker itself is made on the device)
    t.ctx, t.t, t.min_overlap, t.dirty, t.max_lost = None, None, 1, False, 0
    assert t.memory(4) == (None, None) and t.lost() is None
    out = TracksOut()
    assert out.gap_of_region is None and out.memory is None
