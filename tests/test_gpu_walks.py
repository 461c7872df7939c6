"""Long random walks of the tracker on the GPU (tests/walks.py): 48 frames of moving, hiding rectangles and noise bursts with
resets, set_memory calls, empty frames and size changes in between, one tracker handle per walk, every output of every step
against tests/tracks_memory_ref.py with ``==``: track_of_region, table, plane, summary, gap_of_region, the memory summary and the
whole gallery.  What the hand-made sequences of test_gpu_tracks*.py cannot see is state that goes wrong only after several
steps: the gallery's buffer flip, its compaction with survivors of several gaps, claim[] and rclaim[] left over from a larger
frame.  Device buffers carry poisoned guard bytes as in those files; what a call must not write stays poisoned."""
import os
import sys

import numpy as np
import pytest

from infur_amd.processors import Context

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import tracks_memory_ref as M  # noqa: E402
import tracks_ref as T  # noqa: E402
import walks  # noqa: E402
from test_gpu_tracks import OUTS, POISON, Dev, check_step, dev_step  # noqa: E402
from test_gpu_tracks_memory import MEM_OUTS, Tracker, check_memory, memory_dev  # noqa: E402

pytestmark = pytest.mark.gpu


def new_tracker(ctx, case):
    return Tracker(ctx, pair_slots=case.pair_slots, max_lost=case.max_lost, reach=case.reach, gallery_rows=case.gallery_rows)


def describe(case, i, frame, n, rows, got, mem, want):
    """what a failing step's message names: case, frame, op, n, both summaries, both memory summaries"""
    show = lambda a: "not read" if a is None else a.tolist()  # noqa: E731
    return (f"walk {case.name} frame {i} op {frame.op} n {n} table_rows {rows} wanted {frame.want}: summary {show(got['summary'])} (reference "
            f"{show(want.summary)}), memory {show(mem and mem['memory'])} (reference {show(want.memory)})")


def compare(case, i, frame, n, rows, got, mem, want):
    try:
        check_step(got, want, n, rows)
        if mem is not None:
            check_memory(mem, want)
    except AssertionError as e:
        raise AssertionError(f"{describe(case, i, frame, n, rows, got, mem, want)}\n{e}") from e


def as_bytes(got, mem):
    return b"".join(got[name].tobytes() for name in OUTS if got[name] is not None) + b"".join(mem[name].tobytes() for name in MEM_OUTS if mem)


def device_step(ctx, case, ref_steps, log):
    """-> the step of walks.drive for a device tracker: infur_tracks_dev with the outputs the frame wants, then the tracker's memory
    (all of it: it is the state the next steps build on), both against the reference's step; the bytes read are appended to log"""
    def step(trk, i, frame, labels, table, n, rows):
        want = ref_steps[i]
        got = dev_step(ctx, trk, labels, table, n, rows, case.min_overlap, want=frame.want)
        mem = memory_dev(ctx, trk, rows, len(want.gallery) + 2) if want.memory is not None else None
        compare(case, i, frame, n, rows, got, mem, want)
        log.append(as_bytes(got, mem))
    return step


def run_device(ctx, case, trk=None, ref_steps=None):
    """the whole walk on one handle (a new one unless given) -> the bytes of every step"""
    own = trk is None
    trk = new_tracker(ctx, case) if own else trk
    try:
        log = []
        for _ in walks.drive(case, trk, device_step(ctx, case, ref_steps or walks.run_reference(case), log)):
            pass
        assert len(log) == case.frames
        return log
    finally:
        if own:
            trk.close()


_ALONE = {}


def alone(ctx, case):
    """the bytes of a walk run alone on a new handle of the session's context, computed once and shared"""
    if case.name not in _ALONE:
        _ALONE[case.name] = run_device(ctx, case)
    return _ALONE[case.name]


@pytest.mark.parametrize("case", walks.CASES, ids=lambda c: c.name)
def test_walk_equals_the_reference(ctx, case):
    s = walks.stats(case)
    print(f"{case.name} {case.h}x{case.w}: revived {s['revived']} lost {s['lost']} expired {s['expired']}, {s['full_steps']} full and "
          f"{s['mixed_steps']} mixed-gap steps, ops {s['ops']}")
    alone(ctx, case)


def test_two_trackers_interleaved_on_one_context(ctx):
    a, b = walks.BY_NAME["mixed"], walks.BY_NAME["small_gallery"]
    ta, tb = new_tracker(ctx, a), new_tracker(ctx, b)
    try:
        la, lb = [], []
        ga = walks.drive(a, ta, device_step(ctx, a, walks.run_reference(a), la))
        gb = walks.drive(b, tb, device_step(ctx, b, walks.run_reference(b), lb))
        for _ in zip(ga, gb):  # a step of the one, a step of the other
            pass
        assert len(la) == len(lb) == 48
    finally:
        ta.close()
        tb.close()
    assert la == alone(ctx, a) and lb == alone(ctx, b)


def test_a_reused_tracker_equals_a_fresh_one():
    """no_reach to its end, reset(0) and set_memory, then mixed on the same handle: the reference models what counts on (the frame
    counter: BORN and SEEN are 48 later) and says that nothing else differs from a new tracker's walk"""
    first, case = walks.BY_NAME["no_reach"], walks.BY_NAME["mixed"]
    ref = walks.new_reference(first)
    walks.reference_steps(first, ref)
    ref.reset(0)
    ref.set_memory(case.max_lost, case.reach, case.gallery_rows)
    reused, fresh = walks.reference_steps(case, ref), walks.run_reference(case)
    for i, (a, b) in enumerate(zip(reused, fresh)):
        later = b.table.copy()
        later[later[:, T.ID] != T.NONE, T.BORN] += first.frames
        assert (a.table == later).all() and (a.track_of_region == b.track_of_region).all() and (a.plane == b.plane).all(), i
        assert a.summary.tolist() == b.summary.tolist() and (a.memory is None) == (b.memory is None), i
        if a.memory is not None:
            later = b.gallery.copy()
            later[:, (M.L_BORN, M.L_SEEN)] += first.frames
            assert a.memory.tolist() == b.memory.tolist() and (a.gap_of_region == b.gap_of_region).all() and (a.gallery == later).all(), i
    with Context(device=0) as c:  # a context of its own for both: the fresh handle is the first thing its context sees
        alone_bytes = run_device(c, case)  # (compared with the new tracker's reference inside)
    with Context(device=0) as c:
        trk = new_tracker(c, first)
        try:
            run_device(c, first, trk)
            trk.reset(0)
            trk.set_memory(case.max_lost, case.reach, case.gallery_rows)
            again = run_device(c, case, trk, reused)  # (compared with the reused tracker's reference inside)
        finally:
            trk.close()
    assert len(again) == len(alone_bytes) == case.frames


def test_walk_through_regions_on_the_device(ctx):
    """the class planes through infur_regions_dev; labels, table and count stay in device memory and go to infur_tracks_dev as they
    are, on one context for all 48 frames.  The reference: tracks_memory_ref over regions_ref.label"""
    case = walks.BY_NAME["mixed"]
    ref_steps, L = walks.run_reference(case), ctx.L
    keep = [c for c in range(R.WORDS) if c != R.SUM_CONF]  # (no confidence plane is given: SUM_CONF is 0, and Tracks does not read it)

    def step(trk, i, frame, labels, table, n, rows):
        h, w = labels.shape
        hw, want = h * w, ref_steps[i]
        d = Dev(ctx, klass=hw, labels=hw * 4, table=rows * 80, n=4, tor=rows * 4, plane=hw * 4, ttab=rows * 64, summary=16)
        try:
            if hw:
                d.put("klass", frame.plane)
            ctx.check(L.infur_regions_dev(ctx.h, d.ptr["klass"], None, h, w, 8, 0, 0, d.ptr["labels"], d.ptr["table"], rows, d.ptr["n"]))
            p = lambda name: d.ptr[name] if name in frame.want else None  # noqa: E731
            ctx.check(L.infur_tracks_dev(trk.t, d.ptr["labels"], d.ptr["table"], rows, d.ptr["n"], h, w, case.min_overlap, p("tor"), p("plane"),
                                         p("ttab"), p("summary")))
            ctx.synchronize()
            k = min(n, rows)
            assert int(d.get("n").view(np.uint32)[0]) == n and (d.get("labels").view(np.uint32).reshape(h, w) == labels).all(), f"Regions, frame {i}"
            tab = d.get("table").view(np.uint64).reshape(rows, R.WORDS)
            assert (tab[:k, keep] == table[:k, keep]).all() and (tab[:k, R.SUM_CONF] == 0).all() and (tab[k:].view(np.uint8) == POISON).all(), f"Regions, frame {i}"
            got = {"tor": d.get("tor").view(np.uint32), "plane": d.get("plane").view(np.uint32).reshape(h, w),
                   "ttab": d.get("ttab").view(np.uint64).reshape(rows, 8), "summary": d.get("summary").view(np.uint32)}
            for name in OUTS:
                if name not in frame.want:
                    assert (got[name].view(np.uint8) == POISON).all(), f"frame {i}: {name} was not wanted and was written"
                    got[name] = None
        finally:
            d.free()
        mem = memory_dev(ctx, trk, rows, len(want.gallery) + 2) if want.memory is not None else None
        compare(case, i, frame, n, rows, got, mem, want)

    trk = new_tracker(ctx, case)
    try:
        assert sum(1 for _ in walks.drive(case, trk, step)) == case.frames
    finally:
        trk.close()


def test_walks_are_repeatable(ctx):
    """three runs on new handles: the atomics of insert, choose and keep arrive in another order each time, the bytes do not move"""
    case = walks.BY_NAME["small_gallery"]
    runs = [alone(ctx, case), run_device(ctx, case), run_device(ctx, case)]
    assert runs[1] == runs[0] and runs[2] == runs[0]
