"""What the egress stages' host-pointer entry points agree on, one table row per entry point (as tests/test_gpu_frame_rules.py does
for the six calls before them).  The per-stage files pin each stage's results; this file pins, uniformly, the rules the stages
share:

  * the read-back of ``infur_outlines``, ``infur_simplify`` and ``infur_coverage``: how many records and vertices reach the
    caller's arrays -- min(count, rows), and no record at all when the status says that nothing was produced -- and that
    everything behind them is left alone;
  * the faults of ``infur_frame_runs``, ``infur_frame_outlines``, ``infur_frame_polygons`` and ``infur_frame_coverage``, that a
    failing call leaves the context usable, and the no-model rule: the Scale stage still runs and nothing else is written."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_ref as V  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import simplify_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xC5C5C5C5
TOL16 = 12
STAGES = ("outlines", "simplify", "coverage")
COUNT_WORDS = {"outlines": 3, "simplify": _lib.SIMPLIFY_COUNT_WORDS, "coverage": _lib.COVERAGE_COUNT_WORDS}
TRUNCATED = {"simplify": _lib.SIMPLIFY_TRUNCATED, "coverage": _lib.COVERAGE_TRUNCATED}


def p(a):
    return a.ctypes.data if a is not None else None


@functools.lru_cache(maxsize=None)
def cases():
    """[(plane, Outlines' (loops, vertices, counts))] of the two planes: computed once, shared, never changed"""
    return [(k, O.outline(k)) for k in (R.smooth(65, 130), R.stripes(7, 65))]


def reference(stage, plane, outl, loops_rows_in=None):
    l, v, c = outl
    if stage == "outlines":
        return outl
    if stage == "simplify":
        return S.simplify(l, v, c, plane.shape[1], TOL16, loops_rows_in=loops_rows_in)
    return V.coverage(plane, l, v, c, TOL16, loops_rows_in=loops_rows_in)


def host_call(ctx, stage, plane, outl, lo, lrows, vo, vrows, co, loops_rows_in=None):
    (l, v, c), (h, w) = outl, plane.shape
    lin = len(l) if loops_rows_in is None else loops_rows_in
    if stage == "outlines":
        return ctx.L.infur_outlines(ctx.h, p(plane), plane.itemsize, h, w, 0, 0, 0, p(lo), lrows, p(vo), vrows, p(co))
    if stage == "simplify":
        return ctx.L.infur_simplify(ctx.h, p(l), lin, p(v), len(v), p(c), h, w, TOL16, p(lo), lrows, p(vo), vrows, p(co))
    return ctx.L.infur_coverage(ctx.h, p(plane), plane.itemsize, h, w, 0, 0, p(l), lin, p(v), len(v), p(c), TOL16, 0, p(lo), lrows, p(vo), vrows, p(co))


def test_read_back_rules_of_the_three_polygon_calls(ctx):
    """(a) capacities two rows above the counts: the prefix is the reference's, the tail still the canary; (b) one record and
    three vertices of capacity: exactly those are written and the counts are the full ones; (c) Simplify and Coverage with the
    input declared one record short: the truncated bit, counts[0] as the device reports it, no record and -- min(counts[1], rows)
    being 0 -- no vertex"""
    bad = []
    for stage in STAGES:
        for plane, outl in cases():
            rl, rv, rc = reference(stage, plane, outl)
            nl, nv, words = len(rl), len(rv), COUNT_WORDS[stage]
            assert nl >= 2 and nv >= 4 and len(rc) == words
            lo, vo, co = np.full((nl + 2, 4), CANARY, np.uint32), np.full(nv + 2, CANARY, np.uint32), np.full(words, CANARY, np.uint32)
            rows = {"a": (nl + 2, nv + 2, None), "b": (1, 3, None)}
            if stage in TRUNCATED:
                rows["c"] = (nl, nv, len(outl[0]) - 1)
            for case, (lrows, vrows, lin) in rows.items():
                lo[:], vo[:], co[:] = CANARY, CANARY, CANARY
                rc_call = host_call(ctx, stage, plane, outl, lo, lrows, vo, vrows, co, loops_rows_in=lin)
                print(f"{stage:9s} {plane.shape} ({case}) rc {rc_call} counts {co.tolist()}")
                if case == "c":
                    cut = reference(stage, plane, outl, loops_rows_in=lin)
                    want_counts = [len(outl[0]), 0, 0, TRUNCATED[stage]] + [0] * (words - 4)
                    ok = cut[2].tolist() == want_counts and len(cut[0]) == 0 and len(cut[1]) == 0  # (the reference agrees)
                    wl = wv = 0
                else:
                    want_counts, ok = rc.tolist(), True
                    wl, wv = min(nl, lrows), min(nv, vrows)
                ok = ok and rc_call == _lib.OK and co.tolist() == want_counts
                ok = ok and (lo[:wl] == rl[:wl]).all() and (lo[wl:] == CANARY).all() and (vo[:wv] == rv[:wv]).all() and (vo[wv:] == CANARY).all()
                if not ok:
                    bad.append((stage, plane.shape, case, rc_call, co.tolist(), want_counts))
    assert not bad, bad


# --------------------------------------------------------------------------- #
# the four host-pointer frame calls
# --------------------------------------------------------------------------- #
H, WID = 48, 64
NPIX = H * WID
ENTRIES = ("runs", "outlines", "polygons", "coverage")
FRAME_COUNT_WORDS = {"runs": 1, "outlines": 3, "polygons": _lib.SIMPLIFY_COUNT_WORDS, "coverage": _lib.COVERAGE_COUNT_WORDS}
VALID = dict(factor=1.0, outs=True, stats=True, stats_cap=None, scaled=False)
# fault -> (changes to VALID, code, message of infur_last_error or None where there is none to compare); stats_cap -1: one below
# the class count
FAULTS = {
    "stats one class short": (dict(stats_cap=-1), _lib.E_CAPACITY, "the statistics table needs {k} classes, buffer has {k1}"),
    "no stats": (dict(stats=False, stats_cap=0), _lib.OK, None),
    "all outputs null": (dict(outs=False, stats=False, stats_cap=0), _lib.E_INVALID_ARG, "no output wanted: {nothing}"),
    "negative factor": (dict(factor=-1.0), _lib.E_INVALID_SCALE, "Cannot scale by negative number"),
}
NOTHING = {"runs": "runs (with rows), row_start or n_runs", "outlines": "loops (with rows), vertices (with rows) or counts",
           "polygons": "loops_out (with rows), vertices_out (with rows) or counts_out",
           "coverage": "loops_out (with rows), vertices_out (with rows) or counts_out"}


class Outs:
    """the caller's arrays of one frame call, canary-filled: records, vertices or the row index, counts, statistics, scaled frame"""

    def __init__(self, entry, k):
        self.entry = entry
        self.records = np.empty((NPIX, 3 if entry == "runs" else 4), np.uint32)
        self.second = np.empty(H + 1 if entry == "runs" else 4 * NPIX + (H + 1) * (WID + 1), np.uint32)  # row_start | vertices
        self.counts = np.empty(FRAME_COUNT_WORDS[entry], np.uint32)
        self.stats = np.empty((k, _lib.STAT_WORDS), np.uint64)
        self.scaled = np.empty((H, WID, 3), np.uint8)
        self.fill()

    def arrays(self):
        return (self.records, self.second, self.counts, self.stats, self.scaled)

    def fill(self):
        for a in self.arrays():
            a.view(np.uint8)[...] = 0xC5

    def untouched(self, a):
        return bool((a.view(np.uint8) == 0xC5).all())


def invoke(c, o, frame, k, ow, oh, **changes):
    s = dict(VALID, **changes)
    out = lambda a: p(a) if s["outs"] else None  # noqa: E731
    cap = k if s["stats_cap"] is None else (k - 1 if s["stats_cap"] < 0 else s["stats_cap"])
    head = (c.h, p(frame), WID, H, s["factor"], 0, _lib.DECODE_RAW, 0, 0)
    tail = (p(o.stats) if s["stats"] else None, cap, p(o.scaled) if s["scaled"] else None, C.byref(ow), C.byref(oh))
    if o.entry == "runs":
        return c.L.infur_frame_runs(*head, out(o.records), NPIX, out(o.second), H + 1, out(o.counts), *tail)
    body = (out(o.records), NPIX, out(o.second), len(o.second), out(o.counts))
    if o.entry == "outlines":
        return c.L.infur_frame_outlines(*head, 0, *body, *tail)
    return getattr(c.L, "infur_frame_" + o.entry)(*head, 0, 16, *body, *tail)


@pytest.fixture(scope="module")
def frame():
    return W.synth_frame(H, WID, index=1)


def test_fault_table_over_the_four_frame_calls(ctx, model, frame):
    """every fault answers its code and its message on every entry point, and the next valid call on the same context is OK"""
    k = model.get_info().num_classes
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    bad = []
    for entry in ENTRIES:
        o = Outs(entry, k)
        assert invoke(ctx, o, frame, k, ow, oh) == _lib.OK and (ow.value, oh.value) == (WID, H), entry
        for name, (changes, code, msg) in FAULTS.items():
            rc = invoke(ctx, o, frame, k, ow, oh, **changes)
            print(f"{entry:9s} {name:22s} rc {rc:3d}  last_error {ctx.last_error()!r}")
            if rc != code or (msg is not None and ctx.last_error() != msg.format(k=k, k1=k - 1, nothing=NOTHING[entry])):
                bad.append((entry, name, rc, code, ctx.last_error()))
            if invoke(ctx, o, frame, k, ow, oh) != _lib.OK or (ow.value, oh.value) != (WID, H):  # the context is not poisoned
                bad.append((entry, name, "the next valid call failed", ctx.last_error()))
    assert not bad, bad


def test_no_model_rule_over_the_four_frame_calls(frame, oracle):
    """no model: E_MODEL_NOT_LOADED and "no model loaded", after the Scale stage has run -- the scaled frame is the oracle's, and
    every other output still holds its canary"""
    rc, ref = oracle.scale(frame, 0.5, 0)
    assert rc == 0
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    with Context(device=0) as c:
        for entry in ENTRIES:
            o = Outs(entry, 21)
            assert invoke(c, o, frame, 21, ow, oh, factor=0.5, scaled=True) == _lib.E_MODEL_NOT_LOADED, entry
            assert (ow.value, oh.value) == (WID // 2, H // 2) and c.last_error() == "no model loaded", entry
            n = ref.size
            assert (o.scaled.ravel()[:n] == ref.ravel()).all() and o.untouched(o.scaled.ravel()[n:]), entry
            for a in (o.records, o.second, o.counts, o.stats):
                assert o.untouched(a), entry
