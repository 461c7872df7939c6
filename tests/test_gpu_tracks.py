"""Tracks on the GPU: ``infur_tracks*`` and the fused ``infur_frame_tracks*`` against tests/tracks_ref.py, frame by frame over
sequences of planes.  Everything is an integer and fully determined by the planes, so every comparison is ``==`` on whole
arrays.  Device buffers carry poisoned guard bytes; what a call must not write stays poisoned.

The overflow rule as the header states it (R counts runs along rows cut every 64 columns) makes a plane of a single region
65 rows high and 130 columns wide 195 runs: a 64-slot tracker overflows on it by that rule, and the reference says so.  The
cases "tracks normally after an overflow" and "single -> single does not overflow" therefore run with 512 slots at 65 x 130
(195 runs: 390 <= 512) and with 64 slots on planes of at most 32 runs."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd, Tracks, TracksCmd, TracksOut, track_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import tracks_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = T.NONE
GUARD = 64
POISON = 0xA5


class Dev:
    """device buffers with GUARD poisoned bytes behind each; the whole buffer is poisoned before every run"""

    def __init__(self, ctx, **sizes):
        self.ctx, self.sizes, self.ptr = ctx, sizes, {}
        for name, n in sizes.items():
            d = C.c_void_p(None)
            ctx.check(ctx.L.infur_dev_alloc(ctx.h, n + GUARD, C.byref(d)))
            self.ptr[name] = d
        self.poison()

    def poison(self, *names):
        for name in names or self.sizes:
            n = self.sizes[name] + GUARD
            buf = np.full(n, POISON, np.uint8)
            self.ctx.check(self.ctx.L.infur_memcpy_h2d(self.ctx.h, self.ptr[name], buf.ctypes.data, n))

    def put(self, name, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.sizes[name]
        if arr.nbytes:
            self.ctx.check(self.ctx.L.infur_memcpy_h2d(self.ctx.h, self.ptr[name], arr.ctypes.data, arr.nbytes))

    def get(self, name):
        """-> the buffer's bytes; asserts that the guard behind it is intact"""
        n = self.sizes[name]
        b = np.empty(n + GUARD, np.uint8)
        self.ctx.check(self.ctx.L.infur_memcpy_d2h(self.ctx.h, b.ctypes.data, self.ptr[name], n + GUARD))
        assert (b[n:] == POISON).all(), f"the guard bytes behind {name} were overwritten"
        return b[:n].copy()

    def free(self):
        for d in self.ptr.values():
            self.ctx.check(self.ctx.L.infur_dev_free(self.ctx.h, d))


OUTS = ("tor", "plane", "ttab", "summary")
SIZES = ((65, 130), (270, 480))
EDGE_SIZES = ((1, 1), (1, 300), (300, 1), (33, 3), (2, 64), (64, 128))


@functools.lru_cache(maxsize=None)
def regions_of_family(name, h, w):
    """the Regions outputs of every frame of a sequence, computed once and shared: ((labels, table, n), ...)"""
    out = tuple(T.regions_of(k) for k in T.FAMILIES[name](h, w))
    for labels, table, _ in out:
        labels.setflags(write=False)
        table.setflags(write=False)
    return out


class Tracker:
    """an infur_tracker handle"""

    def __init__(self, ctx, max_regions=0, pair_slots=0):
        self.ctx, self.t = ctx, C.c_void_p()
        ctx.check(ctx.L.infur_tracker_create(ctx.h, max_regions, pair_slots, C.byref(self.t)))

    def reset(self, first_id=0):
        self.ctx.check(self.ctx.L.infur_tracker_reset(self.t, first_id))

    def close(self):
        self.ctx.L.infur_tracker_destroy(self.t)


def dev_step(ctx, trk, labels, table, n, rows, min_overlap=1, want=OUTS):
    """infur_tracks_dev on poisoned device buffers -> {name: what the buffer holds, None when not wanted}; rows: table_rows"""
    h, w = labels.shape
    hw = h * w
    d = Dev(ctx, labels=hw * 4, table=rows * 80, n=4, tor=rows * 4, plane=hw * 4, ttab=rows * 64, summary=16)
    try:
        tab = np.full((rows, 10), 0xA5A5A5A5A5A5A5A5, np.uint64)
        tab[:min(n, rows)] = table[:min(n, rows)]
        d.put("labels", labels)
        d.put("table", tab)
        d.put("n", np.array([n], np.uint32))
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_tracks_dev(trk.t, d.ptr["labels"], d.ptr["table"], rows, d.ptr["n"], h, w, min_overlap, p("tor"), p("plane"),
                                         p("ttab"), p("summary")))
        ctx.synchronize()
        got = {"tor": d.get("tor").view(np.uint32), "plane": d.get("plane").view(np.uint32).reshape(h, w),
               "ttab": d.get("ttab").view(np.uint64).reshape(rows, 8), "summary": d.get("summary").view(np.uint32)}
        assert (d.get("labels").view(np.uint32) == labels.ravel()).all() and (d.get("table").view(np.uint64) == tab.ravel()).all()  # inputs
        for name in OUTS:
            if name not in want:
                assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
                got[name] = None
        return got
    finally:
        d.free()


def check_step(got, ref, n, rows, where=""):
    k = min(n, rows)
    if got["summary"] is not None:
        assert got["summary"].tolist() == ref.summary.tolist(), where
    if got["tor"] is not None:
        assert (got["tor"][:k] == ref.track_of_region).all(), where
        assert (got["tor"][k:].view(np.uint8) == POISON).all(), f"{where}: rows at or beyond min(n, table_rows) were written"
    if got["ttab"] is not None:
        assert (got["ttab"][:k] == ref.table).all(), where
        assert (got["ttab"][k:].view(np.uint8) == POISON).all(), f"{where}: rows at or beyond min(n, table_rows) were written"
    if got["plane"] is not None:
        assert (got["plane"] == ref.plane).all(), where


def run_sequence(ctx, name, h, w, spare=3):
    trk, ref = Tracker(ctx), T.Tracker()
    try:
        for i, (labels, table, n) in enumerate(regions_of_family(name, h, w)):
            rows = n + spare
            want = ref.step(labels, table, n, rows)
            # default slots: no plane of these tests may overflow, so a silent "all new" can never pass as a match
            assert 2 * want.runs <= T.DEFAULT_SLOTS and not want.summary[T.STATUS], (name, h, w, i)
            print(f"{name} {labels.shape[0]}x{labels.shape[1]} frame {i}: {n} regions, {want.runs} runs, summary {want.summary.tolist()}")
            check_step(dev_step(ctx, trk, labels, table, n, rows), want, n, rows, f"{name} {h}x{w} frame {i}")
    finally:
        trk.close()


# --------------------------------------------------------------------------- #
# 1. infur_tracks_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(T.FAMILIES))
def test_sequences_equal_the_reference(ctx, name, size):
    assert ctx.L.infur_features() & _lib.FEATURE_TRACKS  # (the first line: fails on a library without the feature)
    run_sequence(ctx, name, *size)


@pytest.mark.parametrize("size", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_shapes_equal_the_reference(ctx, size):
    """a row shorter than a wave, one column, one row, one pixel, exactly one wave-row, whole tiles"""
    for name in ("noise3", "identical"):
        run_sequence(ctx, name, *size)


@functools.lru_cache(maxsize=None)
def ragged_scan_frames():
    """two 96 x 128 planes of 3-class noise labelled at 4-connectivity: more than 2 * 1024 regions each, no multiple of 64; the
    second is the first with the rows 24 .. 71 drawn again"""
    a = R.noise(96, 128, 3, 0)
    b = a.copy()
    b[24:72] = R.noise(96, 128, 3, 100)[24:72]
    return tuple(T.regions_of(k, R.CONNECT_4) for k in (a, b))


def test_the_new_track_scan_spans_several_blocks_with_ragged_ends(ctx):
    """the ranks of the new tracks cross two boundaries between scan blocks of 1024 regions, the last block and its last wave
    are partly filled, and in the second frame continued and new tracks interleave, more than a block of each"""
    trk, ref = Tracker(ctx), T.Tracker()
    try:
        for i, (labels, table, n) in enumerate(ragged_scan_frames()):
            rows = n + 3
            want = ref.step(labels, table, n, rows)
            status, continued, new, _ = want.summary.tolist()
            print(f"frame {i}: {n} regions, {want.runs} runs, summary {want.summary.tolist()}")
            assert n > 2048 and n % 64 != 0
            assert 2 * want.runs <= T.DEFAULT_SLOTS and n <= T.DEFAULT_REGIONS and not status  # neither overflow nor truncation
            assert (continued, new) == (0, n) if i == 0 else (continued > 1024 and new > 1024)
            check_step(dev_step(ctx, trk, labels, table, n, rows), want, n, rows, f"frame {i}")
    finally:
        trk.close()


def test_the_sequences_do_what_they_are_for(ctx):
    """ids stable and ages 1, 2, 3 on identical frames; the shifted blobs keep their tracks; a cross has h * w pairs"""
    ref = T.Tracker()
    for i, (labels, table, n) in enumerate(regions_of_family("identical", 65, 130)):
        s = ref.step(labels, table, n)
        assert (s.track_of_region == np.arange(n)).all() and (s.table[:, T.AGE] == i + 1).all()
    ref = T.Tracker()
    steps = [ref.step(*f) for f in regions_of_family("shift", 270, 480)]
    assert all(s.summary[T.CONTINUED] > s.summary[T.NEW] for s in steps[1:])
    ref = T.Tracker()
    a, b = [ref.step(*f) for f in regions_of_family("cross", 65, 130)]
    assert b.runs == 65 * 130


def test_each_output_alone(ctx):
    frames = regions_of_family("shift", 65, 130)
    for want in (("tor",), ("plane",), ("ttab",), ("summary",), ("tor", "summary"), ("plane", "ttab")):
        trk, ref = Tracker(ctx), T.Tracker()
        try:
            for labels, table, n in frames[:3]:
                check_step(dev_step(ctx, trk, labels, table, n, n + 2, want=want), ref.step(labels, table, n, n + 2), n, n + 2, str(want))
        finally:
            trk.close()


def test_truncated_by_max_regions_and_by_table_rows(ctx):
    frames = regions_of_family("shift", 65, 130)
    n0 = frames[0][2]
    assert n0 > 12
    for max_regions, rows_of in ((7, lambda n: n + 2), (0, lambda n: 5), (4, lambda n: 9), (0, lambda n: 0)):
        trk, ref = Tracker(ctx, max_regions=max_regions), T.Tracker(max_regions=max_regions)
        try:
            for labels, table, n in frames:
                rows = rows_of(n)
                want = ref.step(labels, table, n, rows)
                assert want.summary[T.STATUS] == T.TRUNCATED and (want.plane == NONE).any()
                check_step(dev_step(ctx, trk, labels, table, n, rows), want, n, rows, f"max_regions {max_regions} rows {rows}")
        finally:
            trk.close()


def test_overflow_is_reported_and_the_frame_still_remembered(ctx):
    noise = regions_of_family("noise3", 65, 130)
    single = T.regions_of(R.single(65, 130))
    for slots in (64, 512):
        trk, ref = Tracker(ctx, pair_slots=slots), T.Tracker(pair_slots=slots)
        try:
            status = []
            for labels, table, n in (noise[0], noise[1], single, single, single):
                want = ref.step(labels, table, n, n + 1)
                status.append(want.summary.tolist())
                check_step(dev_step(ctx, trk, labels, table, n, n + 1), want, n, n + 1, f"{slots} slots")
            # the noise pair overflows and is all new; so does noise -> single (one run per remembered region and row)
            assert status[1] == [T.OVERFLOW, 0, noise[1][2], noise[0][2]] and status[2][T.STATUS] == T.OVERFLOW
            # single -> single is 65 * 3 runs: within 512 slots it tracks normally, from the frame an overflowing step remembered
            assert status[3] == ([0, 1, 0, 0] if slots == 512 else [T.OVERFLOW, 0, 1, 1])
        finally:
            trk.close()
    for h, w in ((2, 64), (1, 300), (1, 1)):  # at most 32 runs: a 64-slot table holds them
        trk, ref = Tracker(ctx, pair_slots=64), T.Tracker(pair_slots=64)
        try:
            labels, table, n = T.regions_of(R.single(h, w))
            for want_summary in ([0, 0, 1, 0], [0, 1, 0, 0], [0, 1, 0, 0]):
                want = ref.step(labels, table, n, 2)
                assert want.summary.tolist() == want_summary
                check_step(dev_step(ctx, trk, labels, table, n, 2), want, n, 2, f"single {h}x{w}")
        finally:
            trk.close()


def test_ids_exhausted_and_reset(ctx):
    frames = regions_of_family("shift", 65, 130)
    trk, ref = Tracker(ctx), T.Tracker()
    try:
        def both(i, first_id=None):
            if first_id is not None:
                trk.reset(first_id)
                ref.reset(first_id)
            labels, table, n = frames[i]
            want = ref.step(labels, table, n, n + 1)
            check_step(dev_step(ctx, trk, labels, table, n, n + 1), want, n, n + 1, f"frame {i} after reset {first_id}")
            return want

        both(0)
        assert frames[1][2] > 14
        assert both(1, 0xFFFFFFF0).summary[T.STATUS] == T.IDS_EXHAUSTED  # more than 14 regions: the ids do not fit
        s = both(2)  # an exhausted step forgets the frame and leaves next_id alone: exhausted again
        assert s.summary.tolist() == [T.IDS_EXHAUSTED, 0, 0, 0] and (s.plane == NONE).all()
        n1 = frames[1][2]
        s = both(1, 0xFFFFFFFE - n1)  # exactly fits: next_id + new == 0xFFFFFFFE, the last id is 0xFFFFFFFD
        assert s.summary.tolist() == [0, 0, n1, 0] and s.track_of_region.max() == 0xFFFFFFFD
        s = both(2)  # continued tracks need no new ids; the new ones of this frame do
        assert s.summary[T.STATUS] == T.IDS_EXHAUSTED
        s = both(3, 1000)
        assert s.track_of_region.tolist() == list(range(1000, 1000 + frames[3][2])) and (s.table[:, T.BORN] == 5).all()
        assert both(3).summary.tolist() == [0, frames[3][2], 0, 0]
    finally:
        trk.close()


def test_an_empty_frame_forgets(ctx):
    labels, table, n = regions_of_family("identical", 65, 130)[0]
    trk, ref = Tracker(ctx), T.Tracker()
    try:
        check_step(dev_step(ctx, trk, labels, table, n, n), ref.step(labels, table, n, n), n, n)
        for shape in ((0, 7), (7, 0)):
            e = np.zeros(shape, np.uint32)
            got = dev_step(ctx, trk, e, np.zeros((0, 10), np.uint64), 0, 3)
            ref.step(e, np.zeros((0, 10), np.uint64), 0, 3)
            assert got["summary"].tolist() == [0, 0, 0, 0] and (got["tor"].view(np.uint8) == POISON).all() and (got["ttab"].view(np.uint8) == POISON).all()
        want = ref.step(labels, table, n, n)
        assert want.summary.tolist() == [0, 0, n, 0] and (want.table[:, T.BORN] == 3).all()
        check_step(dev_step(ctx, trk, labels, table, n, n), want, n, n)
    finally:
        trk.close()


def test_five_runs_give_identical_bytes(ctx):
    frames = regions_of_family("noise3", 270, 480)
    runs = []
    for _ in range(5):
        trk = Tracker(ctx)
        try:
            out = [dev_step(ctx, trk, labels, table, n, n) for labels, table, n in frames]
            runs.append(b"".join(g[name].tobytes() for g in out for name in OUTS))
        finally:
            trk.close()
    assert all(r == runs[0] for r in runs[1:])


def test_argument_errors_touch_nothing(ctx):
    L = ctx.L
    t = C.c_void_p(0x77)
    for slots in (48, 32, 96, (1 << 20) + 1):
        assert L.infur_tracker_create(ctx.h, 0, slots, C.byref(t)) == _lib.E_INVALID_ARG and t.value == 0x77
    assert L.infur_tracker_create(ctx.h, (1 << 24) + 1, 0, C.byref(t)) == _lib.E_INVALID_ARG
    assert L.infur_tracker_create(ctx.h, 0, 0, None) == _lib.E_INVALID_ARG
    trk = Tracker(ctx, 16, 64)
    d = Dev(ctx, buf=4096)
    try:
        p = d.ptr["buf"]
        assert L.infur_tracks_dev(trk.t, p, p, 4, p, 4, 4, 1, None, None, None, None) == _lib.E_INVALID_ARG
        assert L.infur_tracks_dev(trk.t, p, p, 4, p, 65536, 65536, 1, p, p, p, p) == _lib.E_INVALID_ARG
        assert L.infur_tracks_dev(trk.t, p, p, 4, p, 0xFFFFFFFF, 1, 1, p, p, p, p) == _lib.E_INVALID_ARG
        for missing in range(3):
            a = [p, p, p]
            a[missing] = None
            assert L.infur_tracks_dev(trk.t, a[0], a[1], 4, a[2], 4, 4, 1, p, p, p, p) == _lib.E_INVALID_ARG
        ctx.synchronize()
        assert (d.get("buf") == POISON).all()
        host = np.full(64, 7, np.uint32)
        hp = host.ctypes.data
        assert L.infur_tracks(trk.t, hp, hp, 1, 1, 4, 4, 1, None, None, None, None) == _lib.E_INVALID_ARG
        assert L.infur_tracks(trk.t, None, hp, 1, 1, 4, 4, 1, hp, hp, hp, hp) == _lib.E_INVALID_ARG and (host == 7).all()
    finally:
        d.free()
        trk.close()


def test_a_tracker_outlives_its_context_as_an_empty_handle():
    with Context(device=0) as c:
        trk = Tracker(c, 16, 64)
        L = c.L
    assert L.infur_tracker_reset(trk.t, 0) == _lib.E_INVALID_ARG
    L.infur_tracker_destroy(trk.t)


# --------------------------------------------------------------------------- #
# 2. the host-pointer call, the processor, the fused frame path
# --------------------------------------------------------------------------- #
def test_host_pointer_call_and_processor(ctx):
    tr, ref = Tracks(ctx), T.Tracker()
    try:
        for i, (labels, table, n) in enumerate(regions_of_family("shift", 270, 480)):
            out = TracksOut(want_plane=True)
            tr.advance((labels, table, n), out)
            want = ref.step(labels, table, n)
            assert (out.track_of_region == want.track_of_region).all() and (out.table == want.table).all() and (out.plane == want.plane).all()
            assert out.summary.tolist() == want.summary.tolist() and (out.status, out.continued, out.new, out.ended) == tuple(want.summary.tolist())
        recs = track_summary(table, out.table, n, 480, 270)
        assert len(recs) == n and [r["track"] for r in recs] == want.track_of_region.tolist()
        moved = [r["step"] for r in recs if r["step"] is not None]
        assert moved and np.median([s[0] for s in moved]) == pytest.approx(2.0, abs=0.5) and np.median([s[1] for s in moved]) == pytest.approx(1.0, abs=0.5)
        # the caller's rows beyond min(n, table_rows) are left alone; a truncated table; reset through the processor
        labels, table, n = regions_of_family("shift", 270, 480)[0]
        tr.control(TracksCmd.Reset(50))
        ref.reset(50)
        want = ref.step(labels, table[:4], n)
        tor, ttab, summary = np.full(6, 7, np.uint32), np.full((6, 8), 7, np.uint64), np.zeros(4, np.uint32)
        tab = np.ascontiguousarray(table[:4])
        ctx.check(ctx.L.infur_tracks(tr.t, labels.ctypes.data, tab.ctypes.data, 4, n, 270, 480, 1, tor.ctypes.data, None, ttab.ctypes.data,
                                     summary.ctypes.data))
        assert (tor[:4] == want.track_of_region).all() and (tor[4:] == 7).all() and (ttab[:4] == want.table).all() and (ttab[4:] == 7).all()
        assert summary.tolist() == want.summary.tolist() == [T.TRUNCATED, 0, 4, 0] and tor[0] == 50
    finally:
        tr.close()


def frame_regions_dev(ctx, d, frame, rows, conn):
    hh, ww = frame.shape[:2]
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    ctx.check(ctx.L.infur_frame_regions_dev(ctx.h, d.ptr["bgr"], ww, hh, 1.0, 0, 1, conn, 0, 0, None, None, 0, d.ptr["labels"], hh * ww * 4,
                                            d.ptr["table"], rows, d.ptr["n"], None, C.byref(ow), C.byref(oh)))


def test_fused_device_call_equals_regions_then_tracks(ctx, model):
    L = ctx.L
    hh, ww, rows = 50, 99, 64
    hw = hh * ww
    frames = [W.synth_frame(hh, ww, index=i) for i in (2, 3, 3)]
    two, one, ref = Tracker(ctx), Tracker(ctx), T.Tracker()
    sizes = dict(tor=rows * 4, plane=hw * 4, ttab=rows * 64, summary=16)
    d = Dev(ctx, bgr=frames[0].nbytes, labels=hw * 4, table=rows * 80, n=4, **sizes)
    e = Dev(ctx, labels=hw * 4, table=rows * 80, n=4, **sizes)
    try:
        for i, frame in enumerate(frames):
            private = i == 2  # the last frame: labels, table and count stay with the tracker
            d.poison()
            e.poison()
            d.put("bgr", frame)
            frame_regions_dev(ctx, d, frame, rows, 8)
            ctx.check(L.infur_tracks_dev(two.t, d.ptr["labels"], d.ptr["table"], rows, d.ptr["n"], hh, ww, 1, d.ptr["tor"], d.ptr["plane"], d.ptr["ttab"],
                                         d.ptr["summary"]))
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            ctx.check(L.infur_frame_tracks_dev(ctx.h, d.ptr["bgr"], ww, hh, 1.0, 0, 1, 8, 0, 0, None, None, 0, None if private else e.ptr["labels"],
                                               0 if private else hw * 4, None if private else e.ptr["table"], rows, None if private else e.ptr["n"],
                                               None, C.byref(ow), C.byref(oh), one.t, 1, e.ptr["tor"], e.ptr["plane"], e.ptr["ttab"], e.ptr["summary"]))
            ctx.synchronize()
            assert (ow.value, oh.value) == (ww, hh)
            for name in ("tor", "plane", "ttab", "summary") + (() if private else ("labels", "table", "n")):
                assert (d.get(name) == e.get(name)).all(), (i, name)
            if private:
                assert all((e.get(name) == POISON).all() for name in ("labels", "table", "n"))
            # ... and both are the reference's answer on the device's own regions
            n = int(d.get("n").view(np.uint32)[0])
            labels, table = d.get("labels").view(np.uint32).reshape(hh, ww), d.get("table").view(np.uint64).reshape(rows, 10)
            want = ref.step(labels, table[:min(n, rows)], n, rows)
            got = {"tor": e.get("tor").view(np.uint32), "plane": e.get("plane").view(np.uint32).reshape(hh, ww),
                   "ttab": e.get("ttab").view(np.uint64).reshape(rows, 8), "summary": e.get("summary").view(np.uint32)}
            check_step(got, want, n, rows, f"frame {i}")
        assert want.summary[T.CONTINUED] == min(n, rows)  # the repeated frame continues every track
    finally:
        d.free()
        e.free()
        two.close()
        one.close()


def test_fused_host_call_equals_the_device_path(ctx, model):
    fp, tr, ref = FramePath(ctx), Tracks(ctx), T.Tracker()
    try:
        for i, idx in enumerate((5, 6, 6)):
            frame = W.synth_frame(61, 97, index=idx)
            r = fp.advance_regions(frame, 1.0, 1, 8, table_rows=48)
            t = fp.advance_tracks(tr, frame, 1.0, 1, 8, table_rows=48, want_plane=True, want_klass=bool(i & 1), want_conf=bool(i & 1), want_labels=i != 2)
            assert t.n == r.n and (t.table == r.table).all() and (t.labels is None or (t.labels == r.labels).all())
            want = ref.step(r.labels, r.table, r.n, 48)
            assert (t.track_of_region == want.track_of_region).all() and (t.track_table == want.table).all() and (t.track_plane == want.plane).all()
            assert t.summary.tolist() == want.summary.tolist()
        L = ctx.L
        ow, oh, buf = C.c_uint32(0), C.c_uint32(0), np.zeros(64, np.uint32)
        p = buf.ctypes.data
        args = (frame.ctypes.data, 97, 61, 1.0, 0, 0, 8, 0, 0, None, None, 0, None, 0, None, 4, None, None, C.byref(ow), C.byref(oh))
        assert L.infur_frame_tracks(ctx.h, *args, tr.t, 1, None, None, None, None) == _lib.E_INVALID_ARG
        assert L.infur_frame_tracks(ctx.h, *args, None, 1, p, None, None, p) == _lib.E_INVALID_ARG
        with Context(device=0) as other:  # a tracker of another context; no model: the Scale stage still runs
            assert L.infur_frame_tracks(other.h, *args, tr.t, 1, p, None, None, p) == _lib.E_INVALID_ARG
            with_t = Tracks(other)
            q = FramePath(other).advance_tracks(with_t, frame, 0.5, want_scaled=True)
            assert q.labels is None and q.summary is None and q.scaled.shape == (30, 48, 3)
            with_t.close()
    finally:
        tr.close()


def test_tracks_calls_leave_the_cached_graphs_alone(blob50):
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
        te, tg, ref = Tracks(ce), Tracks(cg), T.Tracker()  # (created after the capture: a tracker's memory moves no graph)
        for it in range(8):
            fr = frames[it % 4]
            s = fg.advance_tracks(tg, fr, 1.0, 1, 8, table_rows=256, want_plane=bool(it & 1), want_klass=bool(it & 4), want_conf=bool(it & 4))
            e = fe.advance_tracks(te, fr, 1.0, 1, 8, table_rows=256, want_plane=True)
            want = ref.step(e.labels, e.table, e.n, 256)
            assert s.n == e.n and (s.track_table == e.track_table).all() and (e.track_table == want.table).all() and (e.track_plane == want.plane).all()
            assert s.summary.tolist() == want.summary.tolist()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a tracks call caused a capture"
        assert cached1 >= cached0, "a tracks call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the tracks calls were not replayed"
        te.close()
        tg.close()


# --------------------------------------------------------------------------- #
# 3. the command line
# --------------------------------------------------------------------------- #
def test_cli_round_trip(tmp_path):
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames = [W.synth_frame(96, 128, index=i) for i in (0, 0, 1)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    cmd = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip),
           "--tracks", "--regions-out", str(tmp_path / "labels.u32"), "--tracks-out", str(tmp_path / "tracks.u32"), "--max-regions", "40"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = [json.loads(line) for line in r.stdout.splitlines()]
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(3, 96, 128)
    planes = np.frombuffer((tmp_path / "tracks.u32").read_bytes(), np.uint32).reshape(3, 96, 128)
    ref = T.Tracker()
    for i, rec in enumerate(recs):
        assert sorted(rec) == ["classes", "frame", "height", "n_regions", "regions", "tracks", "width"]
        n = rec["n_regions"]
        table = np.zeros((min(n, 40), 10), np.uint64)  # what the reference needs of the rows: class, pixels, sums
        for j, g in enumerate(rec["regions"]):
            table[j, R.CLASS], table[j, R.PIXELS] = g["klass"], g["pixels"]
        want = ref.step(labels[i], table, n, 40)
        assert (planes[i] == want.plane).all(), i
        assert rec["tracks"] == dict(zip(("status", "continued", "new", "ended"), want.summary.tolist()))
        assert [g["track"] for g in rec["regions"]] == want.track_of_region.tolist() and [g["age"] for g in rec["regions"]] == want.table[:, T.AGE].tolist()
        assert all((g["dx"] is None) == (g["age"] == 1) for g in rec["regions"])
    assert recs[1]["tracks"]["new"] == 0 and all(g["dx"] == 0.0 and g["dy"] == 0.0 and g["age"] == 2 for g in recs[1]["regions"])  # the same frame twice
