"""Long random walks of the tracker for the tests: numpy only, no product code, nothing of the GPU at import.

Tracks and its memory are the one decode stage whose answer depends on every earlier call.  A walk is a few dozen frames of
moving, hiding rectangles with bursts of one-pixel noise, interleaved with the calls that forget (reset, set_memory, an empty
frame, another size), stepped through ``tracks_memory_ref.Tracker`` and through the device by ONE driver loop (``drive``): the
sequence of calls is written once, each side applies it to its own tracker object.

``walk`` is a pure function of its arguments through ``np.random.default_rng(seed)``.  ``CASES`` is the table of walks,
``run_reference`` their reference steps (computed once), ``stats`` what tests/test_walks_cpu.py asserts about them.  The seeds
were searched so that every condition of that file holds; the conditions are fixed, the seeds are not.
"""
import collections
import functools

import numpy as np

import regions_ref as R
import tracks_memory_ref as M
import tracks_ref as T

OUTS = ("tor", "plane", "ttab", "summary")
LAST_ID = 0xFFFFFFFE

Frame = collections.namedtuple("Frame", "plane op short want")
Frame.__doc__ = """one frame of a walk: (plane, op) and the step's arguments.  plane: u8 [h, w] class plane, None for the empty
frame; op: None or the call made before the step; short: table_rows = max(1, n // 2) instead of n + 3; want: the wanted outputs"""


def _draw(rects, hh, ww):
    k = np.zeros((hh, ww), np.uint8)
    for r in rects:  # (a later rectangle covers an earlier one; a rectangle that leaves on one side comes back on the other)
        if r["hidden"]:
            continue
        ys = (int(np.floor(r["y"])) + np.arange(min(r["rh"], hh))) % hh
        xs = (int(np.floor(r["x"])) + np.arange(min(r["rw"], ww))) % ww
        k[np.ix_(ys, xs)] = r["klass"]
    return k


def walk(seed, h, w, frames, max_lost=0, reach=0, gallery_rows=0, first_id=None, off_on=False, rects=7, burst_every=10, sprinkle=0.03,
         burst_run=1, ops_at=None):
    """-> [Frame] * frames.  Class 0 is the background (a region like any other: the flags of ``tracks_ref.regions_of``).

    planes   `rects` rectangles of 1 to 3 classes move by a sub-pixel velocity and wrap at the borders; a visible rectangle hides
             with probability 0.25 per frame for 1 .. max(4, max_lost) frames; about every `burst_every` frames, on `burst_run`
             frames in a row, `sprinkle` of the pixels get a class of their own: a burst of one-pixel regions
    ops      each of reset, set_memory, empty and resize once, at drawn frames at least three apart (and `off_on`: memory off,
             then on again two or three frames later, in the place of set_memory); `ops_at`: their frames given, in that order;
             `first_id`: frame 0 starts with reset(first_id)
    steps    5 % have a short table (TRUNCATED), 15 % want a random proper subset of the outputs"""
    rng = np.random.default_rng(seed)
    classes = int(rng.integers(1, 4))
    world = []
    for _ in range(rects):
        world.append(dict(klass=int(rng.integers(1, classes + 1)), rh=int(min(h, rng.integers(min(2, h), max(2, h // 6) + 1))),
                          rw=int(min(w, rng.integers(min(2, w), max(2, w // 6) + 1))), y=float(rng.uniform(0, h)), x=float(rng.uniform(0, w)),
                          vy=float(rng.uniform(-1.2, 1.2)), vx=float(rng.uniform(-1.2, 1.2)), hidden=0))
    # the ops and where they stand
    kinds = ["reset", "off" if off_on else "set_memory", "empty", "resize"]
    rng.shuffle(kinds)
    while True:
        at = np.sort(rng.choice(np.arange(4, frames - 4), size=len(kinds), replace=False))
        if (np.diff(at) >= 3).all():
            break
    if ops_at is not None:
        kinds, at = ["reset", "off" if off_on else "set_memory", "empty", "resize"], np.asarray(ops_at)
    ops, size_of, on_at = {}, {}, None
    for kind, i in zip(kinds, at.tolist()):
        if kind == "reset":
            ops[i] = ("reset", int(rng.integers(0, 1 << 20)))
        elif kind == "set_memory":  # the same parameters or others; never off
            same = rng.random() < 0.5
            ops[i] = ("set_memory", max_lost if same or not max_lost else int(rng.integers(1, max_lost + 2)),
                      reach if same else int(rng.integers(0, 6)), gallery_rows)
        elif kind == "off":
            ops[i] = ("set_memory", 0, int(rng.integers(0, 100)), int(rng.integers(0, 1 << 20)))  # (off: the other two are ignored)
            on_at = i + int(rng.integers(2, 4))
        elif kind == "empty":
            ops[i] = ("empty",)
        else:
            h2, w2 = h, w
            while (h2, w2) == (h, w):
                h2, w2 = max(1, h + int(rng.integers(-3, 4))), max(1, w + int(rng.integers(-5, 6)))
            n = int(rng.integers(2, 4))
            ops[i] = ("resize", h2, w2, n)
            for j in range(i, min(i + n, frames)):
                size_of[j] = (h2, w2)
    if on_at is not None:  # (an op already there moves the return of memory one frame on)
        while on_at in ops:
            on_at += 1
        ops[on_at] = ("set_memory", max_lost, reach, gallery_rows)
    if first_id is not None:
        ops[0] = ("reset", first_id)
    # the bursts
    bursts, i = set(), int(rng.integers(3, burst_every + 1))
    while i < frames:
        bursts.update(range(i, i + burst_run))
        i += burst_run + int(rng.integers(max(1, burst_every - 3), burst_every + 4))
    out = []
    for i in range(frames):
        for r in world:
            if i and not r["hidden"] and rng.random() < 0.25:
                r["hidden"] = int(rng.integers(1, max(4, max_lost) + 1)) + 1
            r["hidden"] = max(0, r["hidden"] - 1)
        hh, ww = size_of.get(i, (h, w))
        k = _draw(world, hh, ww)
        if i in bursts:
            m = rng.random((hh, ww)) < sprinkle
            k[m] = rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)
        for r in world:
            r["y"] += r["vy"]
            r["x"] += r["vx"]
        op = ops.get(i)
        short = bool(rng.random() < 0.05)
        want = OUTS
        if rng.random() < 0.15:
            pick = rng.random(len(OUTS)) < 0.5
            if pick.all() or not pick.any():
                pick[int(rng.integers(len(OUTS)))] ^= True
            want = tuple(name for name, p in zip(OUTS, pick) if p)
        if op == ("empty",):
            k = None
        else:
            k.setflags(write=False)
        out.append(Frame(k, op, short, want))
    return out


# ---------------------------------------------------------------- the case table
_FIELDS = "name seed h w max_lost reach gallery_rows min_overlap first_id pair_slots frames off_on rects burst_every sprinkle burst_run ops_at"
Case = collections.namedtuple("Case", _FIELDS, defaults=(1, None, 0, 48, False, 7, 10, 0.03, 1, None))

CASES = (
    Case("mixed", 0, 33, 96, 3, 2, 0, off_on=True),  # two row tiles of a width that is no multiple of 64
    Case("small_gallery", 45, 65, 130, 4, 1, 8, burst_every=20),
    Case("tiny_gallery", 22, 7, 65, 2, 3, 4),
    Case("no_reach", 1, 48, 200, 5, 0, 0),
    Case("one_row", 0, 1, 300, 3, 4, 0),
    Case("one_col", 0, 300, 1, 3, 4, 0),
    Case("big_reach", 1, 33, 96, 3, 0xFFFFFFFF, 0),  # the 64-bit product and its clamp
    Case("overlap3", 2, 65, 130, 2, 2, 0, min_overlap=3, off_on=True),
    Case("no_memory", 0, 65, 130, 0, 0, 0),  # plain Tracks
    # (the reset that ends the exhausted steps has to follow them closely, and nothing may use up the ids before: the ops are placed)
    Case("near_exhaustion", 5, 33, 96, 3, 2, 0, first_id=LAST_ID - 40, burst_every=30, ops_at=(30, 35, 40, 44)),
    Case("overflow", 2, 65, 130, 2, 2, 0, pair_slots=1024),
    Case("wave_row", 1, 6, 64, 2, 1, 0),  # rows of exactly one wave
    Case("short_row", 1, 9, 33, 2, 1, 0),  # rows shorter than a wave
    Case("scan_blocks", 1, 64, 256, 3, 2, 65536, burst_every=16, sprinkle=0.10, burst_run=3),
)
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def frames_of(case):
    return tuple(walk(case.seed, case.h, case.w, case.frames, case.max_lost, case.reach, case.gallery_rows, case.first_id, case.off_on, case.rects,
                      case.burst_every, case.sprinkle, case.burst_run, case.ops_at))


def _regions(plane, w):
    if plane is None:
        return np.zeros((0, w), np.uint32), np.zeros((0, R.WORDS), np.uint64), 0
    return T.regions_of(plane)


@functools.lru_cache(maxsize=None)
def regions_of(case):
    """the Regions outputs of every frame, computed once and shared: ((labels, table, n), ...); the empty frame: 0 x w"""
    out = tuple(_regions(f.plane, case.w) for f in frames_of(case))
    for labels, table, _ in out:
        labels.setflags(write=False)
        table.setflags(write=False)
    return out


def table_rows(frame, n):
    return max(1, n // 2) if frame.short else n + 3


# ---------------------------------------------------------------- the driver
def drive(case, tracker, step):
    """the one loop both sides run: applies the walk's ops to `tracker` (the reference's or the device's: both have reset and
    set_memory) and yields (i, frame, step(tracker, i, frame, labels, table, n, rows)) frame by frame.  A generator, so that two
    walks can be stepped alternately."""
    for i, (frame, (labels, table, n)) in enumerate(zip(frames_of(case), regions_of(case))):
        if frame.op and frame.op[0] == "reset":
            tracker.reset(frame.op[1])
        elif frame.op and frame.op[0] == "set_memory":
            tracker.set_memory(*frame.op[1:])
        yield i, frame, step(tracker, i, frame, labels, table, n, table_rows(frame, n))


def new_reference(case, memory=True):
    if not memory:
        return M.Tracker(pair_slots=case.pair_slots)
    return M.Tracker(pair_slots=case.pair_slots, max_lost=case.max_lost, reach=case.reach, gallery_rows=case.gallery_rows)


class _NoMemory:
    """a reference tracker whose set_memory only forgets: the same walk as Tracks alone would see it"""

    def __init__(self, ref):
        self.ref = ref

    def reset(self, first_id):
        self.ref.reset(first_id)

    def set_memory(self, *_):
        self.ref.set_memory(0)


def reference_steps(case, tracker):
    """the walk through a given reference tracker -> (MemStep, ...)"""
    step = lambda t, i, frame, labels, table, n, rows: getattr(t, "ref", t).step(labels, table, n, rows, case.min_overlap)  # noqa: E731
    return tuple(s for _, _, s in drive(case, tracker, step))


@functools.lru_cache(maxsize=None)
def run_reference(case):
    """the reference's steps of a walk from a new tracker, computed once and shared: leave them unchanged"""
    return reference_steps(case, new_reference(case))


@functools.lru_cache(maxsize=None)
def run_reference_without_memory(case):
    return reference_steps(case, _NoMemory(new_reference(case, memory=False)))


# ---------------------------------------------------------------- what a walk did, on the reference
def stats(case):
    """per-walk counts of the reference's steps; `held_before[i]`: the gallery's length when step i (and its op) began"""
    frames, steps = frames_of(case), run_reference(case)
    s = dict(revived=0, lost=0, expired=0, gaps=set(), expired_steps=0, mixed_steps=0, all_three_steps=0, full_steps=0, status_steps=0,
             continued_steps=0, truncated_steps=0, overflow_steps=[], exhausted_steps=[], ops_on_a_held_gallery=set(), ops=[], max_lost_step=0,
             max_held=0, held_before=[])
    held = 0
    for i, (f, st) in enumerate(zip(frames, steps)):
        s["held_before"].append(held)
        if f.op:
            s["ops"].append((i, f.op[0]))
            if held:
                s["ops_on_a_held_gallery"].add(f.op[0])
        status = int(st.summary[T.STATUS])
        s["status_steps"] += status != 0
        s["truncated_steps"] += bool(status & T.TRUNCATED)
        s["full_steps"] += bool(status & M.GALLERY_FULL)
        s["continued_steps"] += st.summary[T.CONTINUED] > 0
        if status & T.OVERFLOW:
            s["overflow_steps"].append(i)
        if status & T.IDS_EXHAUSTED:
            s["exhausted_steps"].append(i)
        held = 0
        if st.memory is not None:
            rev, lost, exp, held = (int(v) for v in st.memory)
            s["revived"] += rev
            s["lost"] += lost
            s["expired"] += exp
            s["gaps"].update(int(g) for g in st.gap_of_region if g)
            s["expired_steps"] += exp > 0
            s["mixed_steps"] += len(np.unique(st.gallery[:, M.L_SEEN])) >= 2
            s["all_three_steps"] += bool(rev and lost and exp)
            s["max_lost_step"] = max(s["max_lost_step"], lost)
            s["max_held"] = max(s["max_held"], held)
    return s
