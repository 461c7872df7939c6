"""What a decode stage writes must not depend on what its context ran before (the history invariant, behind the
network).

Segments, Regions, Tracks, Runs, Outlines, Simplify, Coverage, Anchors and Compare each own scratch that only grows and is never
cleared as a whole; a call lays its arrays into it at offsets computed from its arguments and clears exactly the words it
believes it needs.  Every case here runs a TARGET call in a context that has run nothing else and in a context that
tests/stage_history.py walks through the calls that leave the worst bytes behind: a larger plane, a plane one row and one
column larger, the same shape with denser or with empty content, the other element size, the stage's other code path, calls that
stop early and leave their scratch half-written, an empty plane, a rejected call.  All of them are the library's own earlier
calls, through the public API.  Everything the stages write is an exact integer: every comparison is of bytes, fresh against
walked, and of both against the numpy references of tests/ -- "all equal" must not be able to mean "all equally wrong"
(tests/test_stage_history_cpu.py shows that the poisons are poisons)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import anchors_ref as A  # noqa: E402
import compare_ref as CR  # noqa: E402
import coverage_ref as V  # noqa: E402
import history as H  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402
import segments_ref as SR  # noqa: E402
import simplify_ref as S  # noqa: E402
import stage_history as SH  # noqa: E402
import tracks_memory_ref as M  # noqa: E402
from test_gpu_anchors import dev_anchors  # noqa: E402
from test_gpu_compare import OUTPUTS, dev_compare  # noqa: E402
from test_gpu_coverage import dev_coverage  # noqa: E402
from test_gpu_outlines import dev_outlines  # noqa: E402
from test_gpu_regions import Dev, dev_regions  # noqa: E402
from test_gpu_runs import dev_runs  # noqa: E402
from test_gpu_simplify import dev_simplify  # noqa: E402
from test_gpu_tracks import check_step, dev_step  # noqa: E402
from test_gpu_tracks_memory import Tracker, check_memory, memory_dev  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd import weights as W  # noqa: E402
from infur_amd.processors import Context, FramePath, InfurError, Model, ModelCmd, Tracks  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = SH.POISON
NONE = 0xFFFFFFFF


# --------------------------------------------------------------------------- #
# one call of a stage, through the device-pointer and through the host-pointer entry point
# --------------------------------------------------------------------------- #
def run_dev(ctx, c):
    """the ``_dev`` entry point on poisoned, guard-padded device buffers (the helpers of the stages' own test files) -> {output:
    what its buffer holds}; raises InfurError when the call is refused"""
    a, st = SH.args(c), c.stage
    if st == "regions":
        labels, table, n = dev_regions(ctx, a["klass"], a["conf"], a["conn"], a["min_pixels"], a["flags"], table_rows=a["rows"])
        return {"labels": labels, "table": table, "n": np.array([n], np.uint32)}
    if st == "runs":
        runs, row_start, n = dev_runs(ctx, a["plane"], a["flags"], a["skip_value"], rows=a["rows"])
        return {"runs": runs, "row_start": row_start, "n": np.array([n], np.uint32)}
    if st == "outlines":
        got = dev_outlines(ctx, a["plane"], a["flags"], a["skip_value"], a["max_edges"], a["loops_rows"], a["vertex_rows"])
    elif st == "simplify":
        got = dev_simplify(ctx, a["loops"], a["vertices"], a["counts"], a["h"], a["w"], a["tol16"], a["loops_rows_in"], a["vertex_rows_in"],
                           a["loops_rows_out"], a["vertex_rows_out"])
    elif st == "coverage":
        got = dev_coverage(ctx, a["plane"], a["loops"], a["vertices"], a["counts"], a["tol16"], a["skip"], a["loops_rows_in"], a["vertex_rows_in"],
                           a["aug_rows"], a["loops_rows_out"], a["vertex_rows_out"])
    elif st == "anchors":
        dist2, anchors = dev_anchors(ctx, a["plane"], a["flags"], a["skip_value"], rows=a["rows"])
        return {"dist2": dist2, "anchors": anchors}
    elif st == "compare":
        got = dev_compare(ctx, a["a"], a["b"], a["flags"], a["ignore_a"], a["ignore_b"], a["rows_a"], a["rows_b"], a["pair_slots"])
        return {name: got[name] for name in OUTPUTS}
    else:
        raise KeyError(st)
    return dict(zip(("loops", "vertices", "counts"), got))


def padded(arr, rows):
    """a host input array of `rows` rows: what `arr` does not fill holds the poison"""
    arr = np.ascontiguousarray(arr)
    out = SH.filled((rows,) + arr.shape[1:], arr.dtype)
    out[:min(rows, len(arr))] = arr[:rows]
    return out


def run_host(ctx, c):
    """the host-pointer entry point on poisoned host buffers -> {output: what its buffer holds}; raises InfurError when the call is
    refused, after checking that it touched no output"""
    a, st, L, h = SH.args(c), c.stage, ctx.L, ctx.h
    p = lambda x: x.ctypes.data  # noqa: E731
    u32 = np.uint32
    if st == "regions":
        hh, ww = a["klass"].shape
        out = {"labels": SH.filled((hh, ww), u32), "table": SH.filled((a["rows"], 10), np.uint64), "n": SH.filled((1,), u32)}
        rc = L.infur_regions(h, p(a["klass"]), p(a["conf"]), hh, ww, a["conn"], a["min_pixels"], a["flags"], p(out["labels"]), p(out["table"]), a["rows"],
                             p(out["n"]))
    elif st == "runs":
        hh, ww = a["plane"].shape
        out = {"runs": SH.filled((a["rows"], 3), u32), "row_start": SH.filled((hh + 1,), u32), "n": SH.filled((1,), u32)}
        rc = L.infur_runs(h, p(a["plane"]), a["plane"].itemsize, hh, ww, a["flags"], a["skip_value"], p(out["runs"]), a["rows"], p(out["row_start"]),
                          p(out["n"]))
    elif st == "outlines":
        hh, ww = a["plane"].shape
        out = {"loops": SH.filled((a["loops_rows"], 4), u32), "vertices": SH.filled((a["vertex_rows"],), u32), "counts": SH.filled((3,), u32)}
        rc = L.infur_outlines(h, p(a["plane"]), a["plane"].itemsize, hh, ww, a["flags"], a["skip_value"], a["max_edges"], p(out["loops"]), a["loops_rows"],
                              p(out["vertices"]), a["vertex_rows"], p(out["counts"]))
    elif st in ("simplify", "coverage"):
        lin, vin = padded(a["loops"], a["loops_rows_in"]), padded(a["vertices"], a["vertex_rows_in"])
        cin = np.ascontiguousarray(a["counts"][:3], u32)
        words = 4 if st == "simplify" else 6
        out = {"loops": SH.filled((a["loops_rows_out"], 4), u32), "vertices": SH.filled((a["vertex_rows_out"],), u32), "counts": SH.filled((words,), u32)}
        if st == "simplify":
            rc = L.infur_simplify(h, p(lin), a["loops_rows_in"], p(vin), a["vertex_rows_in"], p(cin), a["h"], a["w"], a["tol16"], p(out["loops"]),
                                  a["loops_rows_out"], p(out["vertices"]), a["vertex_rows_out"], p(out["counts"]))
        else:
            rc = L.infur_coverage(h, p(a["plane"]), a["plane"].itemsize, a["h"], a["w"], a["flags"], a["skip"] or 0, p(lin), a["loops_rows_in"], p(vin),
                                  a["vertex_rows_in"], p(cin), a["tol16"], a["aug_rows"], p(out["loops"]), a["loops_rows_out"], p(out["vertices"]),
                                  a["vertex_rows_out"], p(out["counts"]))
    elif st == "anchors":
        hh, ww = a["plane"].shape
        out = {"dist2": SH.filled((hh, ww), u32), "anchors": SH.filled((a["rows"], 2), u32)}
        rc = L.infur_anchors(h, p(a["plane"]), a["plane"].itemsize, hh, ww, a["flags"], a["skip_value"], p(out["dist2"]), p(out["anchors"]), a["rows"])
    elif st == "compare":
        hh, ww = a["a"].shape
        ra, rb = a["rows_a"], a["rows_b"]
        out = {"matrix": SH.filled((ra, rb), u32), "a": SH.filled((ra, 4), u32), "b": SH.filled((rb, 4), u32), "counts": SH.filled((8,), u32)}
        rc = L.infur_compare(h, p(a["a"]), a["a"].itemsize, p(a["b"]), a["b"].itemsize, hh, ww, a["flags"], a["ignore_a"], a["ignore_b"], p(out["matrix"]),
                             ra, rb, p(out["a"]), p(out["b"]), p(out["counts"]), a["pair_slots"])
    else:
        raise KeyError(st)
    if rc != _lib.OK:
        assert all((v.view(np.uint8) == POISON).all() for v in out.values()), f"{SH.tag(c)}: a refused call wrote an output"
        raise InfurError(rc, ctx.last_error())
    return out


def poison(ctx, run, name, c):
    """a poison call -> None, or the sentence of what is wrong with it.  A call that has to stop early or to find nothing must have
    done so (its outputs are the reference's); of the others nothing is looked at beyond the status"""
    if c.expect == "OK":
        got = run(ctx, c)
        return SH.first_difference(SH.expected(c), got) if name in ("STOPPED", "SAME-SPARSE") else None
    try:  # a refused call: its code is looked at like every other step, nothing is asserted before the walk is over
        run(ctx, c)
    except InfurError as e:
        return None if e.code == getattr(_lib, c.expect) else f"returned {e.code} ({e}), not {c.expect}"
    return f"was not refused: {c.expect} expected"


def report(stage, bad):
    """the failure message: how many differences each poison left, then the first forty sentences"""
    tally = {}
    for b in bad:
        key = b.split("] ")[0].lstrip("[")
        tally[key] = tally.get(key, 0) + 1
    return f"{stage}: {len(bad)} differences {tally}:\n" + "\n".join(bad[:40])


def walk_plane_stage(stage, run, entry):
    """every target of a stage: fresh context == reference; then one walked context runs poison -> target for every poison of every
    target.  -> the sentences of what differed (every step is looked at before anything is asserted)"""
    bad, fresh = [], {}
    for t in SH.targets(stage):
        tc = SH.target_call(stage, t)
        with Context(device=0) as c:
            fresh[t] = run(c, tc)
        diff = SH.first_difference(SH.expected(tc), fresh[t])
        if diff is not None:
            bad.append(f"[fresh] {entry} {SH.tag(tc)}: reference against a fresh context -- {diff}")
    steps = 0
    with Context(device=0) as c:
        for t in SH.targets(stage):
            for name, pc, tc in SH.walk_steps(stage, t):
                diff = poison(c, run, name, pc)
                if diff is not None:
                    bad.append(f"[{name} itself] {entry} {SH.tag(pc)}: the poison call -- {diff}")
                got = run(c, tc)
                steps += 1
                for what, ref in (("a fresh context", fresh[t]), ("reference", SH.expected(tc))):
                    diff = SH.first_difference(ref, got)
                    if diff is not None:
                        bad.append(f"[{name}] {entry} {SH.tag(tc)} after {SH.tag(pc)}: {what} against walked -- {diff}")
    print(f"{stage} {entry}: {len(fresh)} targets, {steps} poison -> target steps, {len(bad)} differences")
    return bad


# --------------------------------------------------------------------------- #
# Segments: logits in, four outputs
# --------------------------------------------------------------------------- #
SEG_OUTS = ("klass", "conf", "stats", "rgba")


def segments_dev(ctx, t):
    k, h, w, decode, seed = t
    x = SH.logits(k, h, w, seed)
    hw = h * w
    d = Dev(ctx, x=x.nbytes, klass=hw, conf=hw, stats=k * 64, rgba=hw * 4)
    try:
        d.put("x", x)
        ctx.check(ctx.L.infur_segments_dev(ctx.h, d.ptr["x"], k, h, w, decode, d.ptr["klass"], d.ptr["conf"], d.ptr["stats"], d.ptr["rgba"]))
        ctx.synchronize()
        assert d.get("x").tobytes() == x.tobytes()  # the input is an input
        return {"klass": d.get("klass").reshape(h, w), "conf": d.get("conf").reshape(h, w), "stats": d.get("stats").view(np.uint64).reshape(k, 8),
                "rgba": d.get("rgba").reshape(h, w, 4)}
    finally:
        d.free()


def segments_host(ctx, t):
    k, h, w, decode, seed = t
    x = SH.logits(k, h, w, seed)
    out = {"klass": SH.filled((h, w), np.uint8), "conf": SH.filled((h, w), np.uint8), "stats": SH.filled((k, 8), np.uint64),
           "rgba": SH.filled((h, w, 4), np.uint8)}
    ctx.check(ctx.L.infur_segments(ctx.h, x.ctypes.data, k, h, w, decode, *(out[name].ctypes.data for name in SEG_OUTS)))
    return out


def segments_against_the_oracle(t, got, oracle, tables):
    """the bars of tests/test_gpu_segments.py: RAW is the C oracle's loop, bit for bit; SOFTMAX the float64 reference, the
    confidence byte exact outside the band where an f32 evaluation may truncate to the other side"""
    k, h, w, decode, seed = t
    x = SH.logits(k, h, w, seed)
    if decode == SR.RAW:
        kl, cf = oracle.argmax(x)
        assert (got["klass"] == kl).all() and (got["conf"] == cf).all(), t
        assert (got["stats"] == SR.stats(kl, cf, k)).all() and (got["rgba"] == oracle.colorcode(x)).all(), t
        return
    kl, cf = SR.decode(x, SR.SOFTMAX)
    band = SR.in_band(x)
    diff = got["conf"].astype(int) - cf.astype(int)
    assert (got["klass"] == kl).all() and (diff[~band] == 0).all() and (np.abs(diff) <= 1).all(), t
    assert (got["stats"] == SR.stats(got["klass"], got["conf"], k)).all(), t
    assert (got["rgba"] == tables["color_lut"][got["klass"] % 20, got["conf"]]).all(), t


def walk_segments(run, entry, oracle, tables):
    bad = []
    fresh = {}
    for t in SH.segments_targets():
        with Context(device=0) as c:
            fresh[t] = run(c, t)
        segments_against_the_oracle(t, fresh[t], oracle, tables)
    with Context(device=0) as c:
        for t in SH.segments_targets():
            for name, pt in SH.segments_poisons(t):
                run(c, pt)
                diff = SH.first_difference(fresh[t], run(c, t))
                if diff is not None:
                    bad.append(f"[{name}] {entry} segments {t} after {pt}: a fresh context against walked -- {diff}")
    return bad


# --------------------------------------------------------------------------- #
# Tracks: the tracker's state is history by design
# --------------------------------------------------------------------------- #
def tracks_step_host(trk, labels, table, n, rows, min_overlap, lost_rows):
    """infur_tracks and infur_tracker_memory on poisoned host buffers -> (the step's outputs, the memory's), as dev_step and
    memory_dev give them"""
    ctx, (h, w) = trk.ctx, labels.shape
    tab = SH.filled((rows, 10), np.uint64)
    tab[:min(n, rows)] = table[:min(n, rows)]
    got = {"tor": SH.filled((rows,), np.uint32), "plane": SH.filled((h, w), np.uint32), "ttab": SH.filled((rows, 8), np.uint64),
           "summary": SH.filled((4,), np.uint32)}
    lab = np.ascontiguousarray(labels)
    ctx.check(ctx.L.infur_tracks(trk.t, lab.ctypes.data, tab.ctypes.data, rows, n, h, w, min_overlap, *(got[k].ctypes.data for k in ("tor", "plane", "ttab", "summary"))))
    mem = {"gap": SH.filled((rows,), np.uint32), "memory": SH.filled((4,), np.uint32), "lost": SH.filled((lost_rows, 12), np.uint64)}
    ctx.check(ctx.L.infur_tracker_memory(trk.t, mem["gap"].ctypes.data, rows, mem["memory"].ctypes.data, mem["lost"].ctypes.data, lost_rows))
    return got, mem


def tracks_step(entry, trk, labels, table, n, rows, min_overlap, want):
    """one step through either entry point, every output and the whole gallery against the reference's step -> the bytes read"""
    lost_rows = len(want.gallery) + 2
    if entry == "dev":
        got = dev_step(trk.ctx, trk, labels, table, n, rows, min_overlap)
        mem = memory_dev(trk.ctx, trk, rows, lost_rows)
    else:
        got, mem = tracks_step_host(trk, labels, table, n, rows, min_overlap, lost_rows)
    return got, mem


def tracks_sequence(entry, trk, ref_steps, where, bad):
    """the four-frame sequence on a handle -> {output: bytes} of all steps; differences from the reference go to `bad`"""
    case = SH.tracks_case()
    out = {}
    for i, ((labels, table, n, rows), want) in enumerate(zip(SH.tracks_sequence(), ref_steps)):
        got, mem = tracks_step(entry, trk, labels, table, n, rows, case.min_overlap, want)
        try:
            check_step(got, want, n, rows, f"{where} frame {i}")
            check_memory(mem, want, f"{where} frame {i}")
        except AssertionError as e:
            bad.append(f"[{where}] {entry} frame {i}: the reference against the device -- {e}")
        out.update({f"{i}.{k}": v for k, v in list(got.items()) + list(mem.items())})
    return out


def walk_tracks(entry):
    case, bad = SH.tracks_case(), []
    new = lambda c: Tracker(c, pair_slots=case.pair_slots, max_lost=case.max_lost, reach=case.reach, gallery_rows=case.gallery_rows)  # noqa: E731
    with Context(device=0) as c:
        trk = new(c)
        fresh = tracks_sequence(entry, trk, SH.tracks_reference(), "a new tracker on a fresh context", bad)
        trk.close()
    ref_a, big_steps = SH.tracks_poisoned_reference()
    with Context(device=0) as c:
        a = Tracker(c, max_lost=2, reach=1, gallery_rows=SH.TRACK_BIG_GALLERY)
        for (labels, table, n), want in zip(SH.tracks_big_frames(), big_steps):  # the poison: its summary says that it was one
            got, mem = tracks_step(entry, a, labels, table, n, n + 3, 1, want)
            assert got["summary"].tolist() == want.summary.tolist() and mem["memory"].tolist() == want.memory.tolist()
        assert got["summary"][0] & M.GALLERY_FULL
        b = new(c)
        walked = tracks_sequence(entry, b, SH.tracks_reference(), "a new tracker on a walked context", bad)
        diff = SH.first_difference(fresh, walked)
        if diff is not None:
            bad.append(f"[a new tracker] {entry}: a fresh context against a walked one -- {diff}")
        b.close()
        # the walked handle itself: reset, memory off and on forget everything but the frame counter, which the reference models
        a.reset(0)
        a.set_memory(0)
        a.set_memory(case.max_lost, case.reach, case.gallery_rows)
        ref_a.reset(0)
        ref_a.set_memory(0)
        ref_a.set_memory(case.max_lost, case.reach, case.gallery_rows)
        tracks_sequence(entry, a, SH.tracks_reference(ref_a), "the walked handle after reset and memory off and on", bad)
        a.close()
    return bad


# --------------------------------------------------------------------------- #
# a. b. c.  one case per stage, each on contexts of its own
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("stage", SH.STAGES)
def test_stage_outputs_do_not_depend_on_history(stage, request):
    if stage == "segments":
        oracle, tables = request.getfixturevalue("oracle"), request.getfixturevalue("tables")  # (the other eight need no oracle)
        bad = walk_segments(segments_dev, "dev", oracle, tables) + walk_segments(segments_host, "host", oracle, tables)
    elif stage == "tracks":
        bad = walk_tracks("dev") + walk_tracks("host")
    else:
        bad = walk_plane_stage(stage, run_dev, "dev") + walk_plane_stage(stage, run_host, "host")
    assert not bad, report(stage, bad)


# --------------------------------------------------------------------------- #
# d. the fused frame calls
# --------------------------------------------------------------------------- #
T0 = H.FULL_TARGET  # (75, 109)
FRAME_CALLS = ("segments", "regions", "tracks", "runs", "outlines", "polygons", "coverage", "anchors", "compare")
SHARED = ("outlines", "polygons", "coverage")  # share st_outl, st_outl_plane and st_poly
TOL = 16


def truth_for(size):
    return R.noise(size[0], size[1], 21, seed=size[0])


def frame_call(ctx, name, frame):
    """one infur_frame_* call -> {output: array}; the rows are the plane's worst case, so nothing is truncated"""
    fp = FramePath(ctx)
    hw = frame.shape[0] * frame.shape[1]
    if name == "segments":
        s = fp.advance_segments(frame, 1.0, _lib.DECODE_RAW, want_rgba=True)
        return {"klass": s.klass, "conf": s.conf, "stats": s.stats, "rgba": s.rgba}
    if name == "regions":
        r = fp.advance_regions(frame, 1.0, _lib.DECODE_RAW, 8, 3, 0, table_rows=hw)
        return {"klass": r.klass, "conf": r.conf, "labels": r.labels, "table": r.table, "n": np.array([r.n], np.uint32)}
    if name == "tracks":
        trk = Tracks(ctx)  # a handle of its own: the context is what was walked
        try:
            r = fp.advance_tracks(trk, frame, 1.0, _lib.DECODE_RAW, 8, 3, 0, table_rows=hw, want_plane=True)
        finally:
            trk.close()
        return {"labels": r.labels, "table": r.table, "n": np.array([r.n], np.uint32), "tor": r.track_of_region, "ttab": r.track_table,
                "plane": r.track_plane, "summary": r.summary}
    if name == "runs":
        r = fp.advance_runs(frame, runs_rows=hw)
        return {"runs": r.runs, "row_start": r.row_start, "n": np.array([r.n], np.uint32), "stats": r.stats}
    if name in SHARED:
        r = getattr(fp, "advance_" + name)(frame, **({} if name == "outlines" else {"tol16": TOL}))
        return {"loops": r.loops, "vertices": r.vertices, "counts": np.array(r.counts, np.uint32), "stats": r.stats}
    if name == "anchors":
        r = fp.advance_anchors(frame, 1.0, _lib.DECODE_RAW, 8, 3, 0, table_rows=hw)
        return {"labels": r.labels, "table": r.table, "n": np.array([r.n], np.uint32), "dist2": r.dist2, "anchors": r.anchors}
    if name == "compare":
        r = fp.advance_compare(frame, truth_for(frame.shape[:2]))
        return {"matrix": r.matrix, "a": r.a, "b": r.b, "counts": r.counts}
    raise KeyError(name)


def frame_reference(name, klass, conf):
    """the stage's reference applied to the class plane of a fresh infur_frame_segments -> {output: array} for the outputs it defines"""
    h, w = klass.shape
    if name in ("regions", "tracks", "anchors"):
        rl, rt, rn = R.label(klass, conf, 8, 3, 0)
        out = {"labels": rl, "table": rt, "n": np.array([rn], np.uint32)}
        if name == "tracks":
            st = M.Tracker().step(rl, rt, rn, h * w)
            out.update(tor=st.track_of_region, ttab=st.table, plane=st.plane, summary=st.summary)
        if name == "anchors":
            d = A.distance(rl, A.SKIP, NONE)
            out.update(dist2=d, anchors=A.anchors(rl, d, rn))
        return out
    if name == "runs":
        rr, rrs, rn = U.encode(klass)
        return {"runs": rr, "row_start": rrs, "n": np.array([rn], np.uint32)}
    if name in SHARED:
        l, v, c = O.outline(klass)
        if name == "polygons":
            l, v, c = S.simplify(l, v, c, w, TOL)
        elif name == "coverage":
            l, v, c = V.coverage(klass, l, v, c, TOL)
        return {"loops": l, "vertices": v, "counts": c}
    if name == "compare":
        ref = CR.compare(klass, truth_for((h, w)), 0, 0, 0, W.NUM_CLASSES, W.NUM_CLASSES)
        return {"matrix": ref.matrix, "a": ref.a, "b": ref.b, "counts": ref.counts}
    raise KeyError(name)


def test_frame_calls_do_not_depend_on_history(blob50):
    target = W.synth_frame(T0[0], T0[1], index=H.target_index(T0))
    big = W.synth_frame(H.BIG[0], H.BIG[1], index=H.IDX_BIG)
    bad = []
    with Context(device=0) as c:
        Model(c).control(ModelCmd.LoadBlob(blob50))
        seg = frame_call(c, "segments", target)
    assert len(np.unique(seg["klass"])) > 2  # a class plane with something on it
    fresh = {"segments": seg}
    for name in FRAME_CALLS[1:]:
        with Context(device=0) as c:
            Model(c).control(ModelCmd.LoadBlob(blob50))
            fresh[name] = frame_call(c, name, target)
        ref = frame_reference(name, seg["klass"], seg["conf"])
        diff = SH.first_difference(ref, {k: fresh[name][k] for k in ref})
        if diff is not None:
            bad.append(f"frame {name}: reference against a fresh context -- {diff}")
    assert fresh["regions"]["n"][0] > 1 and fresh["outlines"]["counts"][0] > 1 and fresh["coverage"]["counts"][5] > 0
    with Context(device=0) as c:  # one walked context: BIG through the call, then the target through it
        Model(c).control(ModelCmd.LoadBlob(blob50))
        for name in FRAME_CALLS:
            for before in (name,) + tuple(o for o in SHARED if name in SHARED and o != name):
                frame_call(c, before, big)
                diff = SH.first_difference(fresh[name], frame_call(c, name, target))
                if diff is not None:
                    bad.append(f"frame {name} after the BIG frame through {before}: a fresh context against walked -- {diff}")
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad)
