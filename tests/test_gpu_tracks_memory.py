"""Tracks' memory on the GPU: a tracker with a gallery of lost tracks against tests/tracks_memory_ref.py, frame by frame.  Every
output of every frame is compared with ``==``: track_of_region, plane, table, summary, gap_of_region, the memory summary and
the whole gallery (through ``infur_tracker_memory_dev``).  Device buffers carry poisoned guard bytes; what a call must not
write stays poisoned."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd, Tracks, TracksOut, track_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import tracks_memory_ref as M  # noqa: E402
import tracks_ref as T  # noqa: E402
from test_gpu_tracks import POISON, Dev, check_step  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = ((65, 130), (270, 480))
EDGE_SIZES = ((1, 1), (1, 300), (300, 1), (33, 3), (2, 64), (64, 128))
PARAMS = ((1, 0), (2, 4))
MEM_OUTS = ("gap", "memory", "lost")


class Tracker:
    """an infur_tracker handle, with memory when max_lost is given"""

    def __init__(self, ctx, max_regions=0, pair_slots=0, max_lost=0, reach=0, gallery_rows=0):
        self.ctx, self.t = ctx, C.c_void_p()
        ctx.check(ctx.L.infur_tracker_create(ctx.h, max_regions, pair_slots, C.byref(self.t)))
        if max_lost:
            self.set_memory(max_lost, reach, gallery_rows)

    def set_memory(self, max_lost, reach=0, gallery_rows=0):
        self.ctx.check(self.ctx.L.infur_tracker_set_memory(self.t, max_lost, reach, gallery_rows))

    def reset(self, first_id=0):
        self.ctx.check(self.ctx.L.infur_tracker_reset(self.t, first_id))

    def close(self):
        self.ctx.L.infur_tracker_destroy(self.t)


@functools.lru_cache(maxsize=None)
def regions_of(name, h=0, w=0):
    """the Regions outputs of every frame of a sequence, computed once and shared: ((labels, table, n), ...)"""
    if name == "ragged4":
        out = tuple(M.ragged4(M.ragged_scan_frames()))
    else:
        out = tuple(T.regions_of(k) for k in (M.TIES[name]() if name in M.TIES else M.FAMILIES[name](h, w)))
    for labels, table, _ in out:
        labels.setflags(write=False)
        table.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, h, w, max_lost, reach, gallery_rows=0, spare=3):
    """the reference's steps of a sequence, computed once and shared: (MemStep, ...)"""
    ref = M.Tracker(max_lost=max_lost, reach=reach, gallery_rows=gallery_rows)
    return tuple(ref.step(labels, table, n, n + spare) for labels, table, n in regions_of(name, h, w))


def memory_dev(ctx, trk, rows, lost_rows, want=MEM_OUTS):
    """infur_tracker_memory_dev on poisoned device buffers -> {gap [rows], memory [4], lost [lost_rows, 12]}, None when not wanted"""
    d = Dev(ctx, gap=rows * 4, memory=16, lost=lost_rows * 96)
    try:
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_tracker_memory_dev(trk.t, p("gap"), rows, p("memory"), p("lost"), lost_rows))
        ctx.synchronize()
        got = {"gap": d.get("gap").view(np.uint32), "memory": d.get("memory").view(np.uint32), "lost": d.get("lost").view(np.uint64).reshape(lost_rows, 12)}
        for name in MEM_OUTS:
            if name not in want:
                assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
                got[name] = None
        return got
    finally:
        d.free()


def check_memory(got, ref, where=""):
    """gap_of_region: the reference's below T, 0 up to rows; the gallery: HELD rows, the rows beyond still poisoned"""
    if got["memory"] is not None:
        assert got["memory"].tolist() == ref.memory.tolist(), where
    if got["gap"] is not None:
        t = len(ref.gap_of_region)
        k = min(t, len(got["gap"]))
        assert (got["gap"][:k] == ref.gap_of_region[:k]).all() and (got["gap"][k:] == 0).all(), where
    if got["lost"] is not None:
        k = min(len(ref.gallery), len(got["lost"]))
        assert (got["lost"][:k] == ref.gallery[:k]).all(), where
        assert (got["lost"][k:].view(np.uint8) == POISON).all(), f"{where}: gallery rows at or beyond min(HELD, lost_rows) were written"


def step_both(ctx, trk, frame, want, rows, where=""):
    """one frame through the device tracker, every output against the reference's step `want`"""
    from test_gpu_tracks import dev_step

    labels, table, n = frame
    check_step(dev_step(ctx, trk, labels, table, n, rows), want, n, rows, where)
    if want.memory is not None:
        check_memory(memory_dev(ctx, trk, rows, len(want.gallery) + 2), want, where)


def run_sequence(ctx, name, h, w, max_lost, reach, gallery_rows=0):
    trk = Tracker(ctx, max_lost=max_lost, reach=reach, gallery_rows=gallery_rows)
    try:
        steps = reference(name, h, w, max_lost, reach, gallery_rows)
        for i, (frame, want) in enumerate(zip(regions_of(name, h, w), steps)):
            print(f"{name} {h}x{w} ({max_lost}, {reach}) frame {i}: {frame[2]} regions, summary {want.summary.tolist()}, memory {want.memory.tolist()}")
            step_both(ctx, trk, frame, want, frame[2] + 3, f"{name} {h}x{w} ({max_lost}, {reach}) frame {i}")
        return steps
    finally:
        trk.close()


def revived(steps):
    return sum(int(s.memory[M.REVIVED]) for s in steps)


# --------------------------------------------------------------------------- #
# 1. sequences against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: f"lost{p[0]}_reach{p[1]}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ("gap", "gap2", "flicker", "flicker2", "drift", "shift", "identical", "noise3", "resize"))
def test_sequences_equal_the_reference(ctx, name, size, params):
    assert ctx.L.infur_features() & _lib.FEATURE_TRACK_MEMORY  # (the first line: fails on a library without the feature)
    h, w = size
    # (3-class noise at 270 x 480 loses more than the default 4096 regions a frame: it gets the largest gallery, so that its
    # status is 0 like every other sequence's; test_ragged4 fills a gallery)
    gallery_rows = 65536 if (name, size) == ("noise3", (270, 480)) else 0
    steps = reference(name, h, w, *params, gallery_rows)
    # the reference alone: the sequence does what it is for
    assert all(s.summary[T.STATUS] == 0 for s in steps), "no overflow, truncation or full gallery in these sequences"
    if name in ("gap", "flicker", "flicker2") or (name == "gap2" and params[0] >= 2):
        assert revived(steps) > 0
    if name in ("identical", "drift") or (name == "gap2" and params[0] < 2):
        assert revived(steps) == 0  # (drift: a reach of 0 or 4 pixels does not span h // 2 rows)
    if name == "resize":
        assert len(steps[2].gallery) == 0 and steps[2].memory.tolist() == [0, 0, 0, 0]  # the dimension change empties the gallery
    run_sequence(ctx, name, h, w, *params, gallery_rows)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_drift_within_reach_is_revived(ctx, size):
    h, w = size
    steps = reference("drift", h, w, 1, h // 2)
    assert steps[-1].memory.tolist() == [1, 0, 0, 0] and steps[-1].gap_of_region.tolist() == [0, 1]
    run_sequence(ctx, "drift", h, w, 1, h // 2)


@pytest.mark.parametrize("name,reach,ids,memory", (("two_to_one", 16, [0, 1], [1, 0, 0, 1]), ("two_to_one", 8, [0, 3], [0, 0, 0, 2]),
                                                   ("one_to_two", 16, [0, 1, 2], [1, 0, 0, 0]), ("larger_score", 16, [0, 2, 1], [1, 0, 0, 0]),
                                                   ("other_class", 16, [0, 2], [0, 0, 0, 1])))
def test_ties(ctx, name, reach, ids, memory):
    steps = reference(name, 0, 0, 1, reach)
    assert steps[-1].track_of_region.tolist() == ids and steps[-1].memory.tolist() == memory
    run_sequence(ctx, name, 0, 0, 1, reach)
    for params in PARAMS:  # a reach of 0 or 4 pixels spans none of the 8-pixel gaps between the squares: nobody is revived
        assert revived(reference(name, 0, 0, *params)) == 0
        run_sequence(ctx, name, 0, 0, *params)


@pytest.mark.parametrize("size", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_shapes_equal_the_reference(ctx, size):
    """a row shorter than a wave, one column, one row, one pixel, exactly one wave-row, whole tiles"""
    for name in ("gap", "noise3"):
        for params in PARAMS:
            run_sequence(ctx, name, *size, *params)
    if size == (1, 300):
        assert reference("gap", 1, 300, 1, 0)[-1].memory.tolist() == [2, 0, 0, 0]


@pytest.mark.parametrize("gallery_rows", (0, 64))
def test_ragged4_crosses_scan_blocks_and_fills_the_gallery(ctx, gallery_rows):
    """revived, lost and held each cross a 1,024-element scan block with partly filled last blocks; 64 rows: GALLERY_FULL with
    drops from the front"""
    steps = reference("ragged4", 0, 0, 2, 0, gallery_rows)
    mem = [s.memory.tolist() for s in steps]
    if gallery_rows == 0:
        assert mem[1:] == [[0, 1405, 0, 1405], [1374, 1357, 0, 1388], [1350, 1405, 0, 1443]] and all(s.summary[T.STATUS] == 0 for s in steps)
    else:
        assert [int(s.summary[T.STATUS]) for s in steps] == [0, 8, 8, 8] and [m[M.HELD] for m in mem[1:]] == [64] * 3
        assert [m[M.REVIVED] for m in mem[2:]] == [64, 63]
    run_sequence(ctx, "ragged4", 0, 0, 2, 0, gallery_rows)


def test_five_runs_give_identical_bytes(ctx):
    from test_gpu_tracks import OUTS, dev_step

    runs = []
    for _ in range(5):
        trk = Tracker(ctx, max_lost=2)
        try:
            out = b""
            for labels, table, n in regions_of("ragged4"):
                g = dev_step(ctx, trk, labels, table, n, n)
                m = memory_dev(ctx, trk, n, 4096)
                out += b"".join(g[name].tobytes() for name in OUTS) + b"".join(m[name].tobytes() for name in MEM_OUTS)
            runs.append(out)
        finally:
            trk.close()
    assert all(r == runs[0] for r in runs[1:])


# --------------------------------------------------------------------------- #
# 2. memory off, forgetting, exhaustion, overflow, capacities
# --------------------------------------------------------------------------- #
def test_memory_off_is_tracks(ctx):
    """a tracker that never had set_memory and one after set_memory(0, ...) equal tracks_ref; the memory calls refuse"""
    from test_gpu_tracks import dev_step

    for switched in (False, True):
        for name in ("gap", "noise3"):
            trk, ref = Tracker(ctx, max_lost=2 if switched else 0), T.Tracker()
            d = Dev(ctx, buf=4096)
            try:
                if switched:
                    trk.set_memory(0, 77, 1 << 20)  # (off: the other two arguments are ignored)
                for i, (labels, table, n) in enumerate(regions_of(name, 65, 130)):
                    check_step(dev_step(ctx, trk, labels, table, n, n + 3), ref.step(labels, table, n, n + 3), n, n + 3, f"{name} frame {i}")
                p = d.ptr["buf"]
                assert ctx.L.infur_tracker_memory_dev(trk.t, p, 4, p, p, 4) == _lib.E_INVALID_ARG
                host = np.full(64, 7, np.uint64)
                hp = host.ctypes.data
                assert ctx.L.infur_tracker_memory(trk.t, hp, 4, hp, hp, 4) == _lib.E_INVALID_ARG and (host == 7).all()
                ctx.synchronize()
                assert (d.get("buf") == POISON).all()
            finally:
                d.free()
                trk.close()


def test_argument_errors_touch_nothing(ctx):
    trk = Tracker(ctx, 16, 64, max_lost=1)
    try:
        assert ctx.L.infur_tracker_set_memory(trk.t, 1, 0, 65537) == _lib.E_INVALID_ARG
        assert ctx.L.infur_tracker_set_memory(trk.t, 1, 0xFFFFFFFF, 65536) == _lib.OK
        assert ctx.L.infur_tracker_memory_dev(trk.t, None, 4, None, None, 4) == _lib.E_INVALID_ARG
        assert ctx.L.infur_tracker_memory(trk.t, None, 4, None, None, 4) == _lib.E_INVALID_ARG
        got = memory_dev(ctx, trk, 5, 3)  # before any step: nothing held, no region
        assert got["memory"].tolist() == [0, 0, 0, 0] and (got["gap"] == 0).all() and (got["lost"].view(np.uint8) == POISON).all()
    finally:
        trk.close()


def test_reset_set_memory_and_an_empty_frame_each_empty_the_gallery(ctx):
    frames = regions_of("gap", 65, 130)
    empty = (np.zeros((0, 7), np.uint32), np.zeros((0, 10), np.uint64), 0)
    for how in ("reset", "set_memory", "empty"):
        trk, ref = Tracker(ctx, max_lost=2), M.Tracker(max_lost=2)
        try:
            for i in (0, 1):
                step_both(ctx, trk, frames[i], ref.step(*frames[i], frames[i][2] + 1), frames[i][2] + 1, f"{how} frame {i}")
            assert len(ref.gallery) == 1
            if how == "reset":
                trk.reset(40)
                ref.reset(40)
            elif how == "set_memory":
                trk.set_memory(1, 3, 100)
                ref.set_memory(1, 3, 100)
            else:
                from test_gpu_tracks import dev_step

                got = dev_step(ctx, trk, *empty, 3)
                want = ref.step(*empty, 3)
                assert got["summary"].tolist() == [0, 0, 0, 0] and (got["tor"].view(np.uint8) == POISON).all()
                check_memory(memory_dev(ctx, trk, 3, 2), want, "the empty frame")
            check_memory(memory_dev(ctx, trk, 3, 2), M.MemStep(None, None, None, None, 0, np.zeros(0, np.uint32), np.zeros(4, np.uint32),
                                                              np.zeros((0, 12), np.uint64)), how)
            want = ref.step(*frames[2], frames[2][2] + 1)
            assert want.memory.tolist() == [0, 0, 0, 0] and want.summary.tolist() == [0, 0, 2, 0]  # the bar is new: nothing was held
            step_both(ctx, trk, frames[2], want, frames[2][2] + 1, f"{how}: the frame after")
            want = ref.step(*frames[1], frames[1][2] + 1)
            assert want.memory.tolist() == [0, 1, 0, 1]
            step_both(ctx, trk, frames[1], want, frames[1][2] + 1, f"{how}: memory works on")
        finally:
            trk.close()


def test_ids_exhausted_without_memory_and_not_with_it(ctx):
    """from first_id 0xFFFFFFFC the first frame of gap takes the last two ids; the bar's return needs a third without memory"""
    frames = regions_of("gap", 65, 130)
    first = 0xFFFFFFFE - 2
    for max_lost, last in ((0, [T.IDS_EXHAUSTED, 0, 0, 1]), (1, [0, 1, 0, 0])):
        trk, ref = Tracker(ctx, max_lost=max_lost), M.Tracker(max_lost=max_lost)
        try:
            trk.reset(first)
            ref.reset(first)
            for i, frame in enumerate(frames):
                want = ref.step(*frame, frame[2] + 1)
                step_both(ctx, trk, frame, want, frame[2] + 1, f"max_lost {max_lost} frame {i}")
            assert want.summary.tolist() == last
            if max_lost:
                assert want.memory.tolist() == [1, 0, 0, 0] and want.track_of_region.tolist() == [first, first + 1]
                # ... and an exhausted step with memory empties the gallery: the bar, lost again, cannot return
                for i, frame in enumerate((frames[1], regions_of("noise3", 65, 130)[0])):
                    want = ref.step(*frame, frame[2] + 1)
                    step_both(ctx, trk, frame, want, frame[2] + 1, f"after: frame {i}")
                    assert (i == 1) == bool(want.summary[T.STATUS] & T.IDS_EXHAUSTED)
                    assert i != 1 or (want.memory.tolist() == [0, 0, 0, 0] and len(want.gallery) == 0)
        finally:
            trk.close()


def test_an_overflow_step_follows_the_uniform_rule(ctx):
    """64 slots, the 65 x 130 single-region plane (195 runs): all tracked regions are orphans, all remembered regions end -- and
    the orphan takes its own track back from the gallery one step later"""
    single = T.regions_of(R.single(65, 130))
    small = T.regions_of(R.single(2, 64))
    trk, ref = Tracker(ctx, pair_slots=64, max_lost=1), M.Tracker(pair_slots=64, max_lost=1)
    try:
        seen = []
        for i, frame in enumerate((single, single, single, small, small)):
            want = ref.step(*frame, 2)
            seen.append((want.summary.tolist(), want.memory.tolist()))
            step_both(ctx, trk, frame, want, 2, f"frame {i}")
        assert seen[1] == ([T.OVERFLOW, 0, 1, 1], [0, 1, 0, 1])  # nothing in the gallery yet: new, and the old track is lost
        assert seen[2] == ([T.OVERFLOW, 0, 0, 1], [1, 1, 0, 1])  # the first track returns, the second is lost
        assert seen[4] == ([0, 1, 0, 0], [0, 0, 0, 0])  # 2 x 64: one run, tracks normally
    finally:
        trk.close()


def test_capacities_and_each_output_alone(ctx):
    from test_gpu_tracks import dev_step

    frames = regions_of("flicker", 65, 130)
    steps = reference("flicker", 65, 130, 1, 0, 0, 0)
    trk = Tracker(ctx, max_lost=1)
    try:
        for (labels, table, n), want in zip(frames[:2], steps[:2]):
            check_step(dev_step(ctx, trk, labels, table, n, n), want, n, n)
        held, t = len(want.gallery), len(want.gap_of_region)
        assert held >= 1 and t > 4
        for rows, lost_rows in ((t - 3, held), (t + 5, held + 3), (0, 0), (t, 0)):
            check_memory(memory_dev(ctx, trk, rows, lost_rows), want, f"rows {rows} lost_rows {lost_rows}")
        labels, table, n = frames[2]
        check_step(dev_step(ctx, trk, labels, table, n, n), steps[2], n, n)
        assert steps[2].gap_of_region.max() == 1
        for alone in MEM_OUTS:
            check_memory(memory_dev(ctx, trk, n, 4, want=(alone,)), steps[2], alone)
    finally:
        trk.close()
    # fewer rows than the gallery holds: the rows beyond stay poisoned (ragged4 holds 1405 after its second frame)
    trk = Tracker(ctx, max_lost=2)
    try:
        for (labels, table, n), want in zip(regions_of("ragged4")[:2], reference("ragged4", 0, 0, 2, 0)[:2]):
            dev_step(ctx, trk, labels, table, n, n + 3)
        got = memory_dev(ctx, trk, 10, 1030)
        assert (got["lost"] == want.gallery[:1030]).all() and got["memory"][M.HELD] == 1405
        host = np.full((1500, 12), 7, np.uint64)
        ctx.check(ctx.L.infur_tracker_memory(trk.t, None, 0, None, host.ctypes.data, 1500))
        assert (host[:1405] == want.gallery).all() and (host[1405:] == 7).all()
    finally:
        trk.close()


def test_a_tracker_outlives_its_context_as_an_empty_handle():
    with Context(device=0) as c:
        trk = Tracker(c, 16, 64, max_lost=1)
        L = c.L
    host = np.full(64, 7, np.uint64)
    hp = host.ctypes.data
    assert L.infur_tracker_set_memory(trk.t, 1, 0, 0) == _lib.E_INVALID_ARG
    assert L.infur_tracker_memory(trk.t, hp, 1, hp, hp, 1) == _lib.E_INVALID_ARG and (host == 7).all()
    assert L.infur_tracker_memory_dev(trk.t, hp, 1, hp, hp, 1) == _lib.E_INVALID_ARG
    L.infur_tracker_destroy(trk.t)


# --------------------------------------------------------------------------- #
# 3. the host-pointer call, the processor, the fused frame path
# --------------------------------------------------------------------------- #
def test_host_pointer_call_and_processor(ctx):
    tr, ref = Tracks(ctx, max_lost=1), M.Tracker(max_lost=1)
    plain = Tracks(ctx)
    try:
        for labels, table, n in regions_of("flicker", 65, 130):
            out = TracksOut(want_plane=True)
            tr.advance((labels, table, n), out)
            want = ref.step(labels, table, n)
            assert (out.track_of_region == want.track_of_region).all() and (out.table == want.table).all() and (out.plane == want.plane).all()
            assert out.summary.tolist() == want.summary.tolist() and out.memory.tolist() == want.memory.tolist()
            assert (out.gap_of_region == want.gap_of_region).all() and (tr.lost() == want.gallery).all() and len(tr.lost(0)) == 0
        assert out.memory[_lib.TRACK_MEMORY_REVIVED] == 2
        recs = track_summary(table, out.table, n, 130, 65, gap=out.gap_of_region)
        assert [r["gap"] for r in recs] == want.gap_of_region.tolist() and sum(r["gap"] for r in recs) == 2
        assert all(r["step"] is None for r in recs if r["gap"])  # (a revived track has no remembered region; its PREV_* words are the entry's)
        out = TracksOut()
        plain.advance((labels, table, n), out)
        assert out.gap_of_region is None and out.memory is None and plain.lost() is None
        assert "gap" not in track_summary(table, out.table, n, 130, 65)[0]
    finally:
        tr.close()
        plain.close()


def test_fused_device_call_equals_regions_then_tracks(ctx, model):
    from test_gpu_tracks import frame_regions_dev

    L = ctx.L
    hh, ww, rows = 50, 99, 64
    hw = hh * ww
    frames = [W.synth_frame(hh, ww, index=i) for i in (2, 3, 2, 3)]
    two, one, ref = Tracker(ctx, max_lost=2, reach=4), Tracker(ctx, max_lost=2, reach=4), M.Tracker(max_lost=2, reach=4)
    sizes = dict(tor=rows * 4, plane=hw * 4, ttab=rows * 64, summary=16)
    d = Dev(ctx, bgr=frames[0].nbytes, labels=hw * 4, table=rows * 80, n=4, **sizes)
    e = Dev(ctx, **sizes)
    try:
        for i, frame in enumerate(frames):
            d.poison()
            e.poison()
            d.put("bgr", frame)
            frame_regions_dev(ctx, d, frame, rows, 8)
            ctx.check(L.infur_tracks_dev(two.t, d.ptr["labels"], d.ptr["table"], rows, d.ptr["n"], hh, ww, 1, d.ptr["tor"], d.ptr["plane"], d.ptr["ttab"],
                                         d.ptr["summary"]))
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            ctx.check(L.infur_frame_tracks_dev(ctx.h, d.ptr["bgr"], ww, hh, 1.0, 0, 1, 8, 0, 0, None, None, 0, None, 0, None, rows, None, None,
                                               C.byref(ow), C.byref(oh), one.t, 1, e.ptr["tor"], e.ptr["plane"], e.ptr["ttab"], e.ptr["summary"]))
            ctx.synchronize()
            for name in sizes:
                assert (d.get(name) == e.get(name)).all(), (i, name)
            n = int(d.get("n").view(np.uint32)[0])
            labels, table = d.get("labels").view(np.uint32).reshape(hh, ww), d.get("table").view(np.uint64).reshape(rows, 10)
            want = ref.step(labels, table[:min(n, rows)], n, rows)
            got = {"tor": e.get("tor").view(np.uint32), "plane": e.get("plane").view(np.uint32).reshape(hh, ww),
                   "ttab": e.get("ttab").view(np.uint64).reshape(rows, 8), "summary": e.get("summary").view(np.uint32)}
            check_step(got, want, n, rows, f"frame {i}")
            for trk in (one, two):
                check_memory(memory_dev(ctx, trk, rows, len(want.gallery) + 2), want, f"frame {i}")
            print(f"frame {i}: {n} regions, summary {want.summary.tolist()}, memory {want.memory.tolist()}")
    finally:
        d.free()
        e.free()
        two.close()
        one.close()


def test_cli_round_trip(tmp_path):
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames = [W.synth_frame(96, 128, index=i) for i in (0, 1, 0, 1)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip)]
    r = subprocess.run(base + ["--tracks-memory", "2"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode != 0 and "--tracks" in r.stderr  # both flags need --tracks
    cmd = base + ["--tracks", "--regions-out", str(tmp_path / "labels.u32"), "--tracks-out", str(tmp_path / "tracks.u32"), "--max-regions", "40",
                  "--tracks-memory", "2", "--tracks-reach", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = [json.loads(line) for line in r.stdout.splitlines()]
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(4, 96, 128)
    planes = np.frombuffer((tmp_path / "tracks.u32").read_bytes(), np.uint32).reshape(4, 96, 128)
    ref = M.Tracker(max_lost=2, reach=3)
    for i, rec in enumerate(recs):
        n = rec["n_regions"]
        table = np.zeros((min(n, 40), 10), np.uint64)  # what the reference needs of the rows: class, pixels, box
        for j, g in enumerate(rec["regions"]):
            table[j, R.CLASS], table[j, R.PIXELS], table[j, R.MIN_X:R.MAX_Y + 1] = g["klass"], g["pixels"], g["box"]
        want = ref.step(labels[i], table, n, 40)
        assert (planes[i] == want.plane).all(), i
        assert rec["tracks"] == dict(zip(("status", "continued", "new", "ended", "revived", "lost", "expired", "held"),
                                         want.summary.tolist() + want.memory.tolist()))
        assert [g["track"] for g in rec["regions"]] == want.track_of_region.tolist() and [g["gap"] for g in rec["regions"]] == want.gap_of_region.tolist()


def test_fused_host_call_and_the_cached_graphs(blob50):
    frames = [W.synth_frame(120, 168, index=i) for i in range(4)]
    with Context(device=0) as ce, Context(device=0, graph_replay=True) as cg:
        Model(ce).control(ModelCmd.LoadBlob(blob50))
        Model(cg).control(ModelCmd.LoadBlob(blob50))
        fe, fg = FramePath(ce), FramePath(cg)
        for it in range(10):  # past the capture
            a, _ = fe.advance(frames[it % 4], 1.0)
            b, _ = fg.advance(frames[it % 4], 1.0)
            assert (a == b).all()
        cap0, rep0, cached0 = cg.graph_stats()
        assert cap0 == 1 and cached0 == 1 and rep0 >= 1
        te, tg, ref = Tracks(ce, max_lost=2, reach=8), Tracks(cg), M.Tracker(max_lost=2, reach=8)
        tg.set_memory(2, 8)  # (made after the capture: a tracker's memory moves no graph)
        for it in range(6):
            fr = frames[(0, 1, 0, 1, 2, 0)[it]]
            s = fg.advance_tracks(tg, fr, 1.0, 1, 8, table_rows=256, want_plane=bool(it & 1))
            e = fe.advance_tracks(te, fr, 1.0, 1, 8, table_rows=256, want_plane=True)
            want = ref.step(e.labels, e.table, e.n, 256)
            assert s.n == e.n and (s.track_table == e.track_table).all() and (e.track_table == want.table).all() and (e.track_plane == want.plane).all()
            assert s.summary.tolist() == want.summary.tolist() and s.memory.tolist() == e.memory.tolist() == want.memory.tolist()
            assert (s.gap_of_region == want.gap_of_region).all() and (e.gap_of_region == want.gap_of_region).all()
            assert (tg.lost() == want.gallery).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a tracks call caused a capture"
        assert cached1 >= cached0, "a tracks call dropped a cached graph"
        assert rep1 == rep0 + 6, "the frames between the tracks calls were not replayed"
        te.close()
        tg.close()
