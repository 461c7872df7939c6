"""The walks of tests/walks.py do what they are for, on the reference alone (no GPU): every phase of a step with memory fires in
every walk, with galleries of mixed gaps, and the forgetting calls land on galleries that hold something.  The conditions are
asserted, not the counts: another numpy generator shows up as a condition failing (then the seeds change, never the conditions).
The counts themselves are in LAB_NOTES."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracks_memory_ref as M  # noqa: E402
import tracks_ref as T  # noqa: E402
import walks  # noqa: E402

MEMORY_CASES = [c for c in walks.CASES if c.max_lost]
ids = lambda c: c.name  # noqa: E731


def check_memory_walk(case):
    """the per-walk conditions of a walk with memory"""
    s = walks.stats(case)
    assert s["gaps"] >= set(range(1, case.max_lost + 1)), f"revived at the gaps {sorted(s['gaps'])} only"
    if case.name != "tiny_gallery":  # (there the drops from the front take everything first)
        assert s["expired_steps"] >= 3, s["expired_steps"]
    assert s["mixed_steps"] >= 10, s["mixed_steps"]
    assert s["all_three_steps"] >= 1
    assert s["ops_on_a_held_gallery"] >= {"reset", "set_memory", "empty", "resize"}, s["ops_on_a_held_gallery"]


def check_gallery_full(case):
    s = walks.stats(case)
    if case.name in ("small_gallery", "tiny_gallery"):
        assert s["full_steps"] >= 5, s["full_steps"]
        # ... and on one of them entries are dropped from the front while others expire and others are revived
        assert any(st.memory is not None and st.summary[T.STATUS] & M.GALLERY_FULL and st.memory[M.REVIVED] and st.memory[M.EXPIRED]
                   for st in walks.run_reference(case))
    elif case.gallery_rows in (0, 65536):  # (the scan-block walk has the largest gallery so that it never fills)
        assert s["full_steps"] == 0, s["full_steps"]


def check_every_step(case):
    for i, st in enumerate(walks.run_reference(case)):
        if not st.summary[T.STATUS] & T.IDS_EXHAUSTED:
            revived = int(st.memory[M.REVIVED]) if st.memory is not None else 0
            assert st.summary[T.CONTINUED] + st.summary[T.NEW] + revived == len(st.track_of_region), i  # (T: max_regions is never the limit)
        else:
            assert st.summary[T.CONTINUED] == st.summary[T.NEW] == 0 and (st.track_of_region == T.NONE).all(), i


def check_status(case):
    s = walks.stats(case)
    assert 4 * s["status_steps"] <= case.frames, f"{s['status_steps']} steps with a status"
    assert 2 * s["continued_steps"] >= case.frames, f"{s['continued_steps']} steps continue a track"
    if case.name != "near_exhaustion":
        assert not s["exhausted_steps"]
    if case.name != "overflow":
        assert not s["overflow_steps"]


def predicted_exhaustion(case, memory):
    """the steps at which the ids run out, from the header's rule alone: a second tracker walks the same walk from a small first
    id, where no id can run out, and reports how many NEW ids each step needs; next_id is counted here.  A step whose NEW does
    not fit is exhausted: it leaves next_id alone and forgets the frame and the gallery -- the second tracker is made to forget
    them too (a reset to its own next_id), so that its next step needs what the walk's next step needs"""
    twin = walks.new_reference(case) if memory else walks._NoMemory(walks.new_reference(case, memory=False))
    next_id, out = None, []

    def step(t, i, frame, labels, table, n, rows):
        nonlocal next_id
        t = getattr(t, "ref", t)
        if frame.op and frame.op[0] == "reset":
            next_id = frame.op[1]
            t.reset(1000)
        need = int(t.step(labels, table, n, rows, case.min_overlap).summary[T.NEW])
        if next_id + need > walks.LAST_ID:
            out.append(i)
            t.reset(t.next_id)
        else:
            next_id += need

    for _ in walks.drive(case, twin, step):
        pass
    return out


def check_near_exhaustion(case):
    """the ids run out exactly where the count says, in the middle of the walk, and the walk goes on; memory postpones it: the same
    walk without memory runs out at a step that passes with it"""
    frames, steps = walks.frames_of(case), walks.run_reference(case)
    assert frames[0].op == ("reset", walks.LAST_ID - 40)
    got = [i for i, st in enumerate(steps) if st.summary[T.STATUS] & T.IDS_EXHAUSTED]
    assert got == predicted_exhaustion(case, True) and got and 5 <= got[0] and got[-1] + 6 < case.frames, got
    for i in got:
        assert steps[i].memory.tolist() == [0, 0, 0, 0] and len(steps[i].gallery) == 0
    assert steps[got[0] + 1].summary[T.STATUS] & T.IDS_EXHAUSTED == 0 and steps[got[0] + 1].summary[T.NEW] > 0  # the ids left are still given out
    assert steps[-1].summary[T.CONTINUED] > 0
    plain = walks.run_reference_without_memory(case)
    out = [i for i, st in enumerate(plain) if st.summary[T.STATUS] & T.IDS_EXHAUSTED]
    assert out == predicted_exhaustion(case, False)
    early = [i for i in out if i < got[0]]
    assert early, "no step passes with memory that exhausts the ids without it"
    assert sum(int(st.memory[M.REVIVED]) for st in steps[:early[0] + 1]) > 0  # (the ids memory saved are the revived tracks')


def check_overflow(case):
    s = walks.stats(case)
    assert 3 <= len(s["overflow_steps"]) <= case.frames // 2, s["overflow_steps"]


def check_scan_blocks(case):
    steps = walks.run_reference(case)
    assert case.gallery_rows == 65536
    assert max(int(st.memory[M.LOST]) for st in steps) > 1024
    assert any(st.memory[M.HELD] > 1024 and st.memory[M.HELD] % 1024 for st in steps)


def check_walk(case):
    """every condition that applies to `case` (the seed search runs this too)"""
    check_every_step(case)
    check_status(case)
    check_gallery_full(case)
    if case.max_lost:
        check_memory_walk(case)
    if case.name == "near_exhaustion":
        check_near_exhaustion(case)
    if case.name == "overflow":
        check_overflow(case)
    if case.name == "scan_blocks":
        check_scan_blocks(case)


@pytest.mark.parametrize("case", MEMORY_CASES, ids=ids)
def test_every_phase_fires_in_every_walk_with_memory(case):
    check_memory_walk(case)


@pytest.mark.parametrize("case", walks.CASES, ids=ids)
def test_gallery_full_where_it_is_meant(case):
    check_gallery_full(case)


@pytest.mark.parametrize("case", walks.CASES, ids=ids)
def test_every_step_adds_up(case):
    check_every_step(case)


@pytest.mark.parametrize("case", walks.CASES, ids=ids)
def test_status_is_rare_and_tracks_continue(case):
    check_status(case)


def test_near_exhaustion_runs_out_where_the_count_says_and_later_without_memory():
    check_near_exhaustion(walks.BY_NAME["near_exhaustion"])


def test_overflow_on_some_steps_not_most():
    check_overflow(walks.BY_NAME["overflow"])


def test_the_scan_block_walk_crosses_blocks_in_regions_and_gallery():
    check_scan_blocks(walks.BY_NAME["scan_blocks"])


def test_memory_off_and_on_again_occurs():
    for name in ("mixed", "overlap3"):
        case = walks.BY_NAME[name]
        sets = [(i, f.op) for i, f in enumerate(walks.frames_of(case)) if f.op and f.op[0] == "set_memory"]
        assert [op[1] for _, op in sets] == [0, case.max_lost], sets
        off, on = sets[0][0], sets[1][0]
        steps = walks.run_reference(case)
        assert all(st.memory is None for st in steps[off:on]) and steps[on].memory is not None and steps[on].memory.tolist() == [0, 0, 0, 0]
        assert walks.stats(case)["held_before"][off] > 0


def test_the_step_arguments_vary():
    """short tables and subsets of the outputs occur, and the table of a no-memory walk is plain Tracks'"""
    frames = [f for c in walks.CASES for f in walks.frames_of(c)]
    assert any(f.short for f in frames) and any(f.want != walks.OUTS for f in frames)
    assert all(0 < len(f.want) <= len(walks.OUTS) for f in frames)
    assert {name for f in frames if f.want != walks.OUTS for name in walks.OUTS if name not in f.want} == set(walks.OUTS)  # each is left out somewhere
    case = walks.BY_NAME["no_memory"]
    assert all(st.memory is None and st.gallery is None for st in walks.run_reference(case))
    assert walks.stats(case)["truncated_steps"] > 0


def test_walks_are_a_function_of_their_arguments():
    case = walks.BY_NAME["mixed"]
    args = (case.seed, case.h, case.w, case.frames, case.max_lost, case.reach, case.gallery_rows)
    a, b = walks.walk(*args, off_on=True), walks.walk(*args, off_on=True)
    blob = lambda fs: b"".join((f.plane.tobytes() if f.plane is not None else b"-") + repr((f.op, f.short, f.want)).encode() for f in fs)  # noqa: E731
    assert blob(a) == blob(b) == blob(walks.frames_of(case))
    assert blob(walks.walk(case.seed + 1, *args[1:], off_on=True)) != blob(a)
    names = [c.name for c in walks.CASES]
    assert len(set(names)) == len(names)
    for c in walks.CASES:  # planes of the walk's size, but for the frames of a resize and the empty frame
        frames = walks.frames_of(c)
        assert len(frames) == c.frames
        other = sum(f.plane is None or f.plane.shape != (c.h, c.w) for f in frames)
        assert 3 <= other <= 4 and all(f.plane is None or f.plane.dtype == np.uint8 for f in frames)
