"""Helper of tests/test_gpu_stage_history.py and tests/test_stage_history_cpu.py (a plain module, no tests, no GPU code at import
time): the calls a context is walked through before it runs a TARGET call of a decode stage, the reference's answer to each, and
the comparison of what the device then wrote.

What a context computes for a call must depend on the call's arguments only.  The stages behind the network make
the opposite easy: each owns private scratch that only grows and is never cleared as a whole, lays several arrays into it at
offsets computed from the call's arguments, and clears exactly the words it believes it needs.  So every target below is run
directly after a call of the same stage, on the same context, that leaves the worst bytes behind it:

  BIG          noise(136, 248, 21): larger than every target in both sides and in every count; the scratch is allocated once,
               at this size
  NEAR         noise(h+1, w+1, 21): every array's offset moves by a row or a column
  SAME-DENSE   the target's shape with noise(.., 21), before the moderate target: stale data of the same layout behind its arrays
  SAME-SPARSE  the target's shape with one value, skipped: an empty answer before the dense target
  OTHER-ELEM   the same plane in the other element size
  OTHER-FORM   the stage's other code path on the same scratch (connectivity, skip, Compare's dense matrix / pair table)
  STOPPED      a BIG call that ends early by design and leaves its scratch half-written
  EMPTY        an h * w == 0 call
  REJECTED     a call refused for its arguments: it returns its error code and must change nothing

All of them are the library's own earlier calls, through the public API.  A call is a ``Call`` -- plain data; ``args`` resolves
it into the arrays and numbers of the C call, ``expected`` into the bytes every output buffer must hold afterwards (the poison
byte of the buffers where the call must not write).
"""
import collections
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import anchors_ref as A  # noqa: E402
import compare_ref as CR  # noqa: E402
import coverage_ref as V  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402
import simplify_ref as S  # noqa: E402

SHAPES = [
    (33, 65),  # crosses both Regions seams (tile 64x32), one lane in a second wave-row
    (7, 65),
    (2, 130),
    (1, 5),
]
BIG = (136, 248)
CONTENTS = ("moderate", "dense")
STAGES = ("segments", "regions", "tracks", "runs", "outlines", "simplify", "coverage", "anchors", "compare")
PLANE_STAGES = ("regions", "runs", "outlines", "simplify", "coverage", "anchors", "compare")  # the stages whose input is a plane
TAKES_ELEM = ("runs", "outlines", "coverage", "anchors", "compare")  # ... that take elem_bytes
POISON = 0xA5  # the byte every output buffer holds before a call (tests/test_gpu_*.py: Dev)
TARGET_SPARE, POISON_SPARE = 5, 11  # rows beyond the counts: the host calls' staging moves with them
SKIP, CONN8 = 1, 2  # Outlines' flags (Runs', Anchors' and Coverage's SKIP is 1 as well)
TOL16 = 12
ANCHOR_ROWS = 30  # above the 21 class values; the u32 table maps classes 1 and 3 to 0 and 7, everything else far above
# Anchors' poisons declare other rows than the target: the keys' memset and the host staging (anchors in front of dist2, on a
# 256-byte boundary: it moves above 32 rows) are sized by them.  One poison lies below the target's rows.
ANCHOR_ROWS_ABOVE, ANCHOR_ROWS_ELEM, ANCHOR_ROWS_BELOW = 70, 41, 9
DENSE_ROWS, TABLE_ROWS = (21, 21), (64, 65)  # Compare: rows_a * rows_b <= 4096 is the dense matrix, above it the pair table
POISON_DENSE_ROWS, POISON_TABLE_ROWS = (40, 33), (70, 90)  # the poisons of the target's own form: other rows, the same side of the rule

Plane = collections.namedtuple("Plane", "kind h w elem")
Plane.__doc__ = """kind: moderate, dense, big, near, sparse (one value: 3), sparse0 (one value: 0), empty; elem: 1, 4 (2: rejected)"""
Call = collections.namedtuple("Call", "stage plane opts expect")
Call.__doc__ = """one call of a stage: its input plane, its other arguments as sorted (name, value) pairs, the status it returns"""
Target = collections.namedtuple("Target", "shape content elem form")


def call(stage, plane, expect="OK", **opts):
    return Call(stage, plane, tuple(sorted(opts.items())), expect)


def opt(c, name, default=None):
    return dict(c.opts).get(name, default)


def tag(c):
    """a short name of a call for messages"""
    p = c.plane
    return f"{c.stage} {p.kind} {p.h}x{p.w} u{8 * p.elem}" + "".join(f" {k}={v}" for k, v in c.opts)


# ---------------------------------------------------------------- planes
@functools.lru_cache(maxsize=None)
def plane_u8(kind, h, w):
    if kind == "moderate":
        k = R.noise(1, 5, 3) if (h, w) == (1, 5) else R.smooth(h, w, seed=h + w, cell=6)
    elif kind == "dense":
        k = R.noise(h, w, 21, seed=w)
    elif kind in ("big", "near"):
        k = R.noise(h, w, 21)
    elif kind == "sparse":
        k = R.single(h, w)
    elif kind == "sparse0":
        k = R.single(h, w, c=0)
    elif kind == "empty":
        k = np.zeros((h, w), np.uint8)
    else:
        raise KeyError(kind)
    assert k.shape == (h, w)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def plane_of(p):
    k = plane_u8(p.kind, p.h, p.w)
    out = k if p.elem == 1 else U.as_u32(k) if p.elem == 4 else k.astype(np.uint16)
    out.setflags(write=False)
    return out


def moderate(shape, elem=1):
    return Plane("moderate", shape[0], shape[1], elem)


def dense(shape, elem=1):
    return Plane("dense", shape[0], shape[1], elem)


def big(elem=1):
    return Plane("big", BIG[0], BIG[1], elem)


def near(shape, elem=1):
    return Plane("near", shape[0] + 1, shape[1] + 1, elem)


def sparse(shape, elem=1, zero=False):
    return Plane("sparse0" if zero else "sparse", shape[0], shape[1], elem)


def first_value(p):
    return int(plane_of(p)[0, 0])


def partner_of(p):
    """Compare's second plane: the first moved down and right (most pixels keep their class)"""
    a = plane_of(p)
    b = CR.shifted(a, min(1, p.h - 1), min(2, p.w - 1)) if a.size else a.copy()
    b.setflags(write=False)
    return b


# ---------------------------------------------------------------- the references, once per argument set
@functools.lru_cache(maxsize=None)
def outline_of(p, flags=0, skip_value=0):
    res = O.outline(plane_of(p), flags, skip_value)
    for a in res:
        a.setflags(write=False)
    return res


def _skip(c, name="skip"):
    """the skip option of a call -> (on, value): None is off, 'first' the value of the first pixel"""
    s = opt(c, name)
    if s is None:
        return False, 0
    return True, first_value(c.plane) if s == "first" else int(s)


def _rows(c, name, n):
    """a rows option: None is n + spare, 'short' a third of n (truncation), 'one_short' n - 1, else the number itself"""
    r = opt(c, name)
    if r is None:
        return n + opt(c, "spare", TARGET_SPARE)
    if r == "short":
        return max(1, n // 3)
    if r == "one_short":
        return n - 1
    return int(r)


@functools.lru_cache(maxsize=None)
def args(c):
    """the arguments of the C call as a dict: arrays and plain numbers (rows resolved through the reference)"""
    p, st = c.plane, c.stage
    rejected = c.expect != "OK"
    plane = plane_of(p)
    if st == "regions":
        conf = R.conf_for(plane, seed=p.w)
        conn, min_pixels, flags = opt(c, "conn", 8), opt(c, "min_pixels", 3), opt(c, "flags", 0)
        n = 0 if rejected or not plane.size else R.label(plane, None, conn, min_pixels, flags)[2]
        return dict(klass=plane, conf=conf, conn=conn, min_pixels=min_pixels, flags=flags, rows=_rows(c, "rows", n))
    if st == "runs":
        on, sv = _skip(c)
        flags = opt(c, "flags", SKIP if on else 0)
        n = 0 if rejected else U.encode(plane, flags, sv)[2]
        return dict(plane=plane, flags=flags, skip_value=sv, rows=_rows(c, "rows", n))
    if st == "outlines":
        on, sv = _skip(c)
        flags = opt(c, "flags", (SKIP if on else 0) | opt(c, "conn8", 0))
        if rejected or not plane.size:
            nl = nv = ne = 0
        else:
            nl, nv, ne = (int(v) for v in outline_of(p, flags, sv)[2])
        me = opt(c, "max_edges", 0)
        return dict(plane=plane, flags=flags, skip_value=sv, max_edges=ne - 1 if me == "short" else me, loops_rows=_rows(c, "loops_rows", nl),
                    vertex_rows=_rows(c, "vertex_rows", nv))
    if st in ("simplify", "coverage"):
        on, sv = _skip(c)
        oflags = (SKIP if on else 0) | opt(c, "conn8", 0)
        if plane.size:
            loops, vertices, counts = outline_of(Plane(p.kind, p.h, p.w, 1 if p.elem == 2 else p.elem), oflags, sv)
        else:  # an empty plane has no loops
            loops, vertices, counts = np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(3, np.uint32)
        nl, nv = len(loops), len(vertices)
        out = dict(loops=loops, vertices=vertices, counts=counts, h=opt(c, "h", p.h), w=opt(c, "w", p.w), tol16=opt(c, "tol16", TOL16),
                   loops_rows_in=_rows(c, "loops_rows_in", nl), vertex_rows_in=_rows(c, "vertex_rows_in", nv), loops_rows_out=_rows(c, "loops_rows_out", nl))
        if st == "simplify":
            out["vertex_rows_out"] = _rows(c, "vertex_rows_out", nv)
            return out
        aug = opt(c, "aug_rows", 0)
        if aug == "short":
            aug = int(V.coverage(plane, loops, vertices, counts, out["tol16"], SKIP if on else 0, sv)[2][4]) - 1
        out.update(plane=plane, skip=sv if on else None, flags=opt(c, "flags", SKIP if on else 0), aug_rows=aug,
                   vertex_rows_out=_rows(c, "vertex_rows_out", nv + (p.h + 1) * (p.w + 1)))
        return out
    if st == "anchors":
        on, sv = _skip(c)
        return dict(plane=plane, flags=opt(c, "flags", SKIP if on else 0), skip_value=sv, rows=opt(c, "rows", ANCHOR_ROWS))
    if st == "compare":
        rows_a, rows_b = opt(c, "rows", DENSE_ROWS if opt(c, "form", "dense") == "dense" else TABLE_ROWS)
        assert CR.is_dense(rows_a, rows_b) == (opt(c, "form", "dense") == "dense")
        on, sv = _skip(c, "ignore")
        return dict(a=plane, b=partner_of(p), flags=opt(c, "flags", CR.IGNORE_A if on else 0), ignore_a=sv, ignore_b=0, rows_a=rows_a, rows_b=rows_b,
                    pair_slots=opt(c, "pair_slots", 0))
    raise KeyError(st)


def filled(shape, dtype):
    """an output buffer as it is before the call: every byte the poison"""
    n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return np.full(n, POISON, np.uint8).view(dtype).reshape(shape)


def _prefix(shape, dtype, head):
    out = filled(shape, dtype)
    k = min(len(head), shape[0])
    out[:k] = head[:k]
    return out


@functools.lru_cache(maxsize=None)
def expected(c):
    """{output: the bytes its buffer holds after the call}, in the order the stage documents its outputs.  Rows beyond the counts
    (and everything a stopped call must not touch) still hold the poison."""
    assert c.expect == "OK", "a rejected call has no answer"
    a, st = args(c), c.stage
    if st == "regions":
        k = a["klass"]
        if not k.size:
            return {"labels": filled(k.shape, np.uint32), "table": filled((a["rows"], 10), np.uint64), "n": np.zeros(1, np.uint32)}
        rl, rt, rn = R.label(k, a["conf"], a["conn"], a["min_pixels"], a["flags"])
        return {"labels": rl, "table": _prefix((a["rows"], 10), np.uint64, rt), "n": np.array([rn], np.uint32)}
    if st == "runs":
        rr, rrs, rn = U.encode(a["plane"], a["flags"], a["skip_value"])
        return {"runs": _prefix((a["rows"], 3), np.uint32, rr), "row_start": rrs, "n": np.array([rn], np.uint32)}
    if st == "outlines":
        if not a["plane"].size:
            rl, rv, rc = np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32), np.zeros(3, np.uint32)
        else:
            rl, rv, rc = O.outline(a["plane"], a["flags"], a["skip_value"], a["max_edges"])
        return {"loops": _prefix((a["loops_rows"], 4), np.uint32, rl), "vertices": _prefix((a["vertex_rows"],), np.uint32, rv), "counts": rc}
    if st == "simplify":
        rl, rv, rc = S.simplify(a["loops"], a["vertices"], a["counts"], a["w"], a["tol16"], a["loops_rows_in"], a["vertex_rows_in"])
    elif st == "coverage":
        rl, rv, rc = V.coverage(a["plane"], a["loops"], a["vertices"], a["counts"], a["tol16"], a["flags"], a["skip"] or 0, a["loops_rows_in"],
                                a["vertex_rows_in"], a["aug_rows"])
    if st in ("simplify", "coverage"):
        return {"loops": _prefix((a["loops_rows_out"], 4), np.uint32, rl), "vertices": _prefix((a["vertex_rows_out"],), np.uint32, rv), "counts": rc}
    if st == "anchors":
        if not a["plane"].size:
            none = np.zeros((a["rows"], 2), np.uint32)
            none[:, 0] = A.NONE
            return {"dist2": filled(a["plane"].shape, np.uint32), "anchors": none}
        d = A.distance(a["plane"], a["flags"], a["skip_value"])
        return {"dist2": d, "anchors": A.anchors(a["plane"], d, a["rows"])}
    if st == "compare":
        ref = CR.compare(a["a"], a["b"], a["flags"], a["ignore_a"], a["ignore_b"], a["rows_a"], a["rows_b"], a["pair_slots"])
        return {"matrix": ref.matrix, "a": ref.a, "b": ref.b, "counts": ref.counts}
    raise KeyError(st)


# ---------------------------------------------------------------- targets and walks
def elems_of(stage):
    """Regions takes class bytes only; Simplify takes loops, and those of the u32 plane carry its values"""
    return (1,) if stage == "regions" else (1, 4)


def targets(stage):
    forms = ("dense", "table") if stage == "compare" else (None,)
    return [Target(s, content, e, f) for s in SHAPES for content in CONTENTS for e in elems_of(stage) for f in forms]


def target_plane(t):
    return Plane(t.content, t.shape[0], t.shape[1], t.elem)


def target_call(stage, t):
    if stage == "compare":
        return call(stage, target_plane(t), form=t.form)
    return call(stage, target_plane(t))  # Regions: min_pixels 3 (the default of args): with 0 or 1 the per-root counts are never read


def _form_poisons(stage, p, t):
    """OTHER-FORM: the stage's other code paths, on the target's own plane"""
    sp = dict(spare=POISON_SPARE)
    if stage == "regions":
        return [call(stage, p, conn=4, **sp), call(stage, p, flags=R.SKIP_BACKGROUND, **sp), call(stage, p, min_pixels=0, **sp)]
    if stage == "runs":
        return [call(stage, p, skip="first", **sp)]
    if stage == "anchors":
        return [call(stage, p, skip="first", rows=ANCHOR_ROWS_ABOVE)]
    if stage == "outlines":
        return [call(stage, p, conn8=CONN8, **sp), call(stage, p, skip="first", **sp)]
    if stage == "simplify":
        return [call(stage, p, conn8=CONN8, **sp), call(stage, p, tol16=0, **sp)]
    if stage == "coverage":
        return [call(stage, p, conn8=CONN8, **sp), call(stage, p, skip="first", **sp)]
    if stage == "compare":
        if t.form == "dense":
            return [call(stage, p, form="table", pair_slots=64), call(stage, p, form="table")]
        return [call(stage, p, form="dense"), call(stage, p, form="table", pair_slots=64)]
    raise KeyError(stage)


def _stopped_poisons(stage):
    """STOPPED: BIG calls that end early by design"""
    b = big()
    if stage == "regions":
        return [call(stage, b, rows="short")]
    if stage == "runs":
        return [call(stage, b, rows="short")]
    if stage == "outlines":
        return [call(stage, b, max_edges="short", spare=POISON_SPARE)]
    if stage == "simplify":
        return [call(stage, b, loops_rows_in="one_short", spare=POISON_SPARE)]
    if stage == "coverage":
        return [call(stage, b, loops_rows_in="one_short", spare=POISON_SPARE), call(stage, b, aug_rows="short", spare=POISON_SPARE)]
    if stage == "compare":
        return [call(stage, b, form="table", pair_slots=64, rows=POISON_TABLE_ROWS)]
    return []  # Anchors has no early end


def _empty_poisons(stage, t):
    """EMPTY: h = 0.  Coverage alone defines no answer for it (its h and w start at 1: an empty plane is E_INVALID_ARG); Simplify
    takes h = 0 with no loops and answers {0, 0, 0, 0}"""
    if stage == "coverage":
        return []
    e = Plane("empty", 0, t.shape[1], t.elem)
    if stage == "simplify":
        return [call(stage, e, spare=POISON_SPARE)]
    if stage == "compare":
        return [call(stage, e, form=t.form)]
    if stage in ("regions", "runs", "outlines"):
        return [call(stage, e, rows=4)] if stage != "outlines" else [call(stage, e, loops_rows=4, vertex_rows=4)]
    return [call(stage, e)]


def _rejected_poisons(stage, p):
    """REJECTED: an element size of 2 where the stage takes one, and an argument outside its range"""
    bad = "E_INVALID_ARG"
    two = Plane(p.kind, p.h, p.w, 2)
    if stage == "regions":
        return [call(stage, p, bad, conn=5, rows=8), call(stage, p, bad, flags=2, rows=8)]
    if stage == "runs":
        return [call(stage, two, bad, rows=8), call(stage, p, bad, flags=2, rows=8)]
    if stage == "outlines":
        return [call(stage, two, bad, loops_rows=8, vertex_rows=8), call(stage, p, bad, flags=4, loops_rows=8, vertex_rows=8)]
    if stage == "simplify":
        return [call(stage, p, bad, tol16=65536), call(stage, p, bad, w=8192)]
    if stage == "coverage":
        return [call(stage, two, bad), call(stage, p, bad, tol16=65536)]
    if stage == "anchors":
        return [call(stage, two, bad), call(stage, p, bad, flags=2)]
    if stage == "compare":
        return [call(stage, two, bad), call(stage, p, bad, flags=4)]
    raise KeyError(stage)


def poisons(stage, t):
    """[(name, Call)]: every poison of a target, in the order the walk makes them"""
    p = target_plane(t)
    form = dict(form=t.form) if stage == "compare" else {}
    sp = dict(spare=POISON_SPARE)  # other rows than the target's, whatever the counts are
    near_sp = el_sp = sp
    if stage == "anchors":
        sp, near_sp, el_sp = dict(rows=ANCHOR_ROWS_ABOVE), dict(rows=ANCHOR_ROWS_BELOW), dict(rows=ANCHOR_ROWS_ELEM)
    elif stage == "compare":
        sp = near_sp = el_sp = dict(rows=POISON_DENSE_ROWS if t.form == "dense" else POISON_TABLE_ROWS)
    out = [("BIG", call(stage, big(), **form, **sp)), ("NEAR", call(stage, near(t.shape), **form, **near_sp))]
    if t.content == "moderate":
        out.append(("SAME-DENSE", call(stage, dense(t.shape, t.elem), **form, **sp)))
    else:
        skip = {"ignore": "first"} if stage == "compare" else {"flags": R.SKIP_BACKGROUND} if stage == "regions" else {"skip": "first"}
        out.append(("SAME-SPARSE", call(stage, sparse(t.shape, t.elem, zero=stage == "regions"), **form, **skip, **sp)))
    if stage in TAKES_ELEM:
        out.append(("OTHER-ELEM", call(stage, Plane(p.kind, p.h, p.w, 5 - p.elem), **form, **el_sp)))
    out += [("OTHER-FORM", c) for c in _form_poisons(stage, p, t)]
    out += [("STOPPED", c) for c in _stopped_poisons(stage)]
    out += [("EMPTY", c) for c in _empty_poisons(stage, t)]
    out += [("REJECTED", c) for c in _rejected_poisons(stage, p)]
    return out


def walk_steps(stage, t):
    """[(poison name, the poison call, the target call)]: one walked context runs them in this order, the target after each"""
    tc = target_call(stage, t)
    return [(name, pc, tc) for name, pc in poisons(stage, t)]


# ---------------------------------------------------------------- what a plane costs the scratch
@functools.lru_cache(maxsize=None)
def counts(p, skip=False):
    """every count that indexes a stage's scratch, for a u8 plane (skip: with the first pixel's value skipped / ignored)"""
    k = plane_of(p)
    sv = first_value(p)
    fl = SKIP if skip else 0
    if skip:  # (Regions skips class 0 only: its sparse plane holds nothing else)
        regions = R.label(k, None, 8, 0, R.SKIP_BACKGROUND)[2]
    else:
        regions = R.label(k, None, 8)[2]
    loops, vertices, oc = outline_of(p, fl, sv)
    sc = S.simplify(loops, vertices, oc, p.w, TOL16)[2]
    vc = V.coverage(k, loops, vertices, oc, TOL16, fl, sv)[2]
    cc = CR.compare(k, partner_of(p), CR.IGNORE_A if skip else 0, sv, 0, *DENSE_ROWS).counts
    return {"regions": int(regions), "runs": int(U.encode(k, fl, sv)[2]), "n_loops": int(oc[0]), "n_vertices": int(oc[1]), "n_edges": int(oc[2]),
            "kept": int(sc[1]), "n_aug": int(vc[4]), "n_arcs": int(vc[5]), "pairs": int(cc[CR.PAIRS]), "compare_runs": int(cc[CR.RUNS])}


# ---------------------------------------------------------------- Segments: logits instead of a plane
SEG_SHAPES = [(7, 65), (33, 65)]
SEG_CLASSES = (3, 21)
SEG_BIG_K = 40


def logits(k, h, w, seed):
    return np.random.default_rng(seed).normal(0.4, 0.5, size=(k, h, w)).astype(np.float32)


def segments_targets():
    """(k, h, w, decode, seed)"""
    return [(k, h, w, decode, 100 + k + h) for (h, w) in SEG_SHAPES for k in SEG_CLASSES for decode in (0, 1)]


def segments_poisons(t):
    """[(name, (k, h, w, decode, seed))]: more classes, more pixels, the same shape with other content"""
    k, h, w, decode, seed = t
    return [("LARGER-K", (SEG_BIG_K, h, w, decode, 7)), ("BIG", (k, BIG[0], BIG[1], decode, 8)), ("SAME", (k, h, w, decode, seed + 1000)),
            ("OTHER-FORM", (k, h, w, 1 - decode, seed + 2000))]


# ---------------------------------------------------------------- Tracks: the tracker's state is history by design
TRACK_FRAMES = 4
TRACK_BIG_STEPS = 3
TRACK_BIG_GALLERY = 4096  # rows of the poisoning tracker's gallery: a step of noise loses six times as many tracks (GALLERY_FULL)


def tracks_case():
    """tests/walks.py's smallest case"""
    import walks

    return min(walks.CASES, key=lambda c: (c.h * c.w, c.name))


@functools.lru_cache(maxsize=None)
def tracks_sequence():
    """the first four frames of that case as ((labels, table, n, table_rows), ...): no op falls among them"""
    import walks

    case = tracks_case()
    frames = walks.frames_of(case)[:TRACK_FRAMES]
    assert all(f.op is None and f.plane is not None for f in frames)
    return tuple((labels, table, n, n + 3) for labels, table, n in walks.regions_of(case)[:TRACK_FRAMES])


@functools.lru_cache(maxsize=None)
def tracks_big_frames():
    """three BIG noise frames of other content each: nearly every track of one is lost in the next"""
    import tracks_ref as T

    out = tuple(T.regions_of(R.noise(BIG[0], BIG[1], 21, seed=50 + i)) for i in range(TRACK_BIG_STEPS))
    for labels, table, _ in out:
        labels.setflags(write=False)
        table.setflags(write=False)
    return out


def tracks_new_reference():
    import tracks_memory_ref as M

    case = tracks_case()
    return M.Tracker(pair_slots=case.pair_slots, max_lost=case.max_lost, reach=case.reach, gallery_rows=case.gallery_rows)


def tracks_reference(tracker=None):
    """the sequence through a reference tracker (a new one unless given) -> (MemStep, ...)"""
    case = tracks_case()
    ref = tracker or tracks_new_reference()
    return tuple(ref.step(labels, table, n, rows, case.min_overlap) for labels, table, n, rows in tracks_sequence())


def tracks_poisoned_reference():
    """the reference of the handle that poisons: memory on, three BIG steps that overfill the gallery -> (tracker, its steps)"""
    import tracks_memory_ref as M

    ref = M.Tracker(max_lost=2, reach=1, gallery_rows=TRACK_BIG_GALLERY)
    return ref, tuple(ref.step(labels, table, n, n + 3) for labels, table, n in tracks_big_frames())


# ---------------------------------------------------------------- comparison
def first_difference(a, b):
    """None when two results ({output: array}) are the same bytes; otherwise a sentence naming the first output (in a's order)
    that differs, the number of elements that differ, the first index and the two values there."""
    for k in a:
        if k not in b:
            return f"{k}: missing on one side"
        if a[k] is None or b[k] is None:
            if a[k] is not b[k]:
                return f"{k}: None on one side"
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        if x.size == 0:
            continue
        ne = (x.reshape(-1).view(np.uint8).reshape(-1, x.itemsize) != y.reshape(-1).view(np.uint8).reshape(-1, x.itemsize)).any(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0])
            idx = tuple(int(v) for v in np.unravel_index(i, x.shape))
            return f"{k}: {int(ne.sum())} of {ne.size} elements differ, first at {idx}: {x.reshape(-1)[i]!r} against {y.reshape(-1)[i]!r}"
    extra = [k for k in b if k not in a]
    return f"{extra[0]}: missing on one side" if extra else None
