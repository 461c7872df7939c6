"""Coverage on the GPU: loop records, vertices and counts of ``infur_coverage*`` and of the fused ``infur_frame_coverage*`` against
tests/coverage_ref.py.  The kept set is a function of the plane and the loops alone, so every comparison is ``==`` on whole
arrays.  Every output buffer is filled with a poison byte first: what a call must leave alone still holds it afterwards, and what
it must write owes nothing to an initialisation."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Coverage, CoverageOut, FramePath, Outlines, OutlinesOut, SimplifyCmd, outlines_by_value, outlines_polygons

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_ref as V  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import test_gpu_outlines as TO  # noqa: E402  (its poisoned, guard-padded device buffers)

pytestmark = pytest.mark.gpu

RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
SKIP, CONN8 = _lib.OUTLINES_SKIP, _lib.OUTLINES_CONN8
NONE = 0xFFFFFFFF
POISON, POISON32 = TO.POISON, TO.POISON32
Dev = TO.Dev
TOLS = (0, 11, 12, 16, 64, 65535)


planes = V.planes


@functools.lru_cache(maxsize=None)
def outlined(conn):
    return [O.outline(k, conn | (SKIP if skip is not None else 0), skip or 0) for _, k, skip, _ in planes()]


@functools.lru_cache(maxsize=None)
def reference(conn, tol16):
    return [V.coverage(k, l, v, c, tol16, V.SKIP if skip is not None else 0, skip or 0) for (_, k, skip, _), (l, v, c) in zip(planes(), outlined(conn))]


def dev_coverage(ctx, plane, loops, vertices, counts, tol16, skip=None, loops_rows_in=None, vertex_rows_in=None, aug_rows=0, loops_rows_out=None,
                 vertex_rows_out=None, want=("loops", "vertices", "counts"), spare=5):
    """infur_coverage_dev on poisoned device buffers -> (loops_out [loops_rows_out, 4], vertices_out [vertex_rows_out], counts_out
    [6]) as the buffers hold them, None for what was not wanted (and that buffer is checked to be untouched).  The input buffers
    hold loops_rows_in records and vertex_rows_in vertices: what the arrays do not fill stays poisoned."""
    plane = np.ascontiguousarray(plane)
    h, w = plane.shape
    loops, vertices = np.asarray(loops, np.uint32).reshape(-1, 4), np.asarray(vertices, np.uint32)
    lin = len(loops) + spare if loops_rows_in is None else loops_rows_in
    vin = len(vertices) + spare if vertex_rows_in is None else vertex_rows_in
    lout = len(loops) + spare if loops_rows_out is None else loops_rows_out
    vout = len(vertices) + (h + 1) * (w + 1) + spare if vertex_rows_out is None else vertex_rows_out
    d = Dev(ctx, plane=plane.nbytes, lin=lin * 16, vin=vin * 4, cin=12, loops=lout * 16, vertices=vout * 4, counts=24)
    try:
        d.put("plane", plane)
        for name, arr, rows in (("lin", loops, lin), ("vin", vertices, vin)):
            buf = np.full(d.sizes[name], POISON, np.uint8)
            part = arr[:rows].reshape(-1).view(np.uint8)
            buf[:len(part)] = part
            d.put(name, buf)
        d.put("cin", np.asarray(list(counts)[:3] + [0] * (3 - min(3, len(counts))), np.uint32))
        before = {name: d.get(name).tobytes() for name in ("plane", "lin", "vin", "cin")}
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_coverage_dev(ctx.h, d.ptr["plane"], plane.itemsize, h, w, _lib.COVERAGE_SKIP if skip is not None else 0, skip or 0, d.ptr["lin"],
                                           lin, d.ptr["vin"], vin, d.ptr["cin"], tol16, aug_rows, p("loops"), lout, p("vertices"), vout, p("counts")))
        ctx.synchronize()
        got = (d.get("loops").view(np.uint32).reshape(lout, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
        assert all(d.get(name).tobytes() == b for name, b in before.items())  # the input is an input
        for name, g in zip(("loops", "vertices", "counts"), got):
            if name not in want:
                assert (g.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return tuple(g if name in want else None for name, g in zip(("loops", "vertices", "counts"), got))
    finally:
        d.free()


def check_result(ref, got, name=""):
    """whole arrays against the reference's; what lies behind the counts still holds the poison"""
    (rl, rv, rc), (loops, vertices, counts) = ref, got
    assert counts.tolist() == rc.tolist(), (name, counts, rc)
    assert (loops[:len(rl)] == rl).all() and (loops[len(rl):] == POISON32).all(), name
    assert (vertices[:len(rv)] == rv).all() and (vertices[len(rv):] == POISON32).all(), name


# --------------------------------------------------------------------------- #
# 1. infur_coverage_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conn", [0, CONN8])
def test_planes_equal_the_reference(ctx, conn):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE  # (the first line: fails on a library without the feature)
    for tol16 in TOLS:
        kept = 0
        for (name, k, skip, ringed), (l, v, c), ref in zip(planes(), outlined(conn), reference(conn, tol16)):
            got = dev_coverage(ctx, k, l, v, c, tol16, skip)
            check_result(ref, got, (name, tol16))
            kept += int(ref[2][1])
            if skip is None:  # the pairing invariant on what the device wrote
                nl, nv = int(got[2][0]), int(got[2][1])
                V.check_invariants(k, got[0][:nl], got[1][:nv], got[2], ringed and V.ring_holds(k.shape, tol16))
        print(f"conn {conn} tol16 {tol16}: {kept} vertices kept")


def test_pinned_counts_on_the_device(ctx):
    """the figures the stage was specified with: input vertices, inserted junctions, kept vertices"""
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    smooth, noise, board = R.smooth(135, 240, seed=750), R.noise(24, 40, 5, seed=3), R.checkerboard(9, 11)
    for plane, nv, inserted, kept in ((smooth, 5168, 218, {0: 5386, 11: 2958, 16: 1240, 64: 899}), (noise, 2618, 335, {0: 2953, 11: 2937, 16: 2723, 64: 2719}),
                                      (board, 396, 0, {16: 392})):
        for conn in (0, CONN8):
            l, v, c = O.outline(plane, conn)
            assert c[1] == nv
            for tol16, n in kept.items():
                counts = dev_coverage(ctx, plane, l, v, c, tol16, want=("counts",))[2]
                assert counts[1] == n and counts[4] == nv + inserted and counts[3] == 0, (conn, tol16, counts)


@pytest.mark.parametrize("conn", [0, CONN8])
def test_outlines_left_on_the_device(ctx, conn):
    """infur_outlines_dev, then infur_coverage_dev on what it left in device memory, rows and all: equal to the host-pointer call"""
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    for i, (name, k, skip, _) in enumerate(planes()):
        if name not in ("smooth", "noise", "labels", "bar 129 ringed", "spiral u32", "saddle with a none"):
            continue
        h, w = k.shape
        l, v, c = outlined(conn)[i]
        lrows, vrows, arows = len(l) + 3, len(v) + 3, len(v) + (h + 1) * (w + 1)
        flags = conn | (SKIP if skip is not None else 0)
        d = Dev(ctx, plane=k.nbytes, lin=lrows * 16, vin=vrows * 4, cin=12, loops=lrows * 16, vertices=arows * 4, counts=24)
        try:
            d.put("plane", k)
            P = d.ptr
            ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["plane"], k.itemsize, h, w, flags, skip or 0, 0, P["lin"], lrows, P["vin"], vrows, P["cin"]))
            for tol16 in (0, 16):
                d.poison("loops", "vertices", "counts")
                ctx.check(ctx.L.infur_coverage_dev(ctx.h, P["plane"], k.itemsize, h, w, flags & SKIP, skip or 0, P["lin"], lrows, P["vin"], vrows, P["cin"], tol16,
                                                   0, P["loops"], lrows, P["vertices"], arows, P["counts"]))
                ctx.synchronize()
                got = (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
                check_result(reference(conn, tol16)[i], got, (name, tol16))
                # the host-pointer call and the processor
                out = CoverageOut()
                Coverage(ctx).control(SimplifyCmd.Tol16(tol16)).advance((k, l, v, c, skip), out)
                rl, rv, rc = reference(conn, tol16)[i]
                assert [out.n_loops, out.n_vertices, out.n_degenerate, out.status, out.n_aug, out.n_arcs] == rc.tolist()
                assert (out.loops == rl).all() and (out.vertices == rv).all()
                assert len(outlines_polygons(out.loops, out.vertices, w)) == len(rl)
                assert sorted(outlines_by_value(out.loops, out.vertices, w)) == sorted(set(l[:, 2].tolist()))
        finally:
            d.free()


# --------------------------------------------------------------------------- #
# 2. calling modes and capacities
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def smooth_case(tol16=12):
    k = R.smooth(65, 130)
    l, v, c = O.outline(k)
    return k, (l, v, c), V.coverage(k, l, v, c, tol16)


def test_every_subset_of_outputs(ctx):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    for want in (("loops",), ("vertices",), ("counts",), ("loops", "counts"), ("vertices", "counts"), ("loops", "vertices")):
        loops, vertices, counts = dev_coverage(ctx, k, l, v, c, 12, want=want, spare=0)
        assert loops is None or (loops[:len(rl)] == rl).all(), want
        assert vertices is None or ((vertices[:len(rv)] == rv).all() and (vertices[len(rv):] == POISON32).all()), want
        assert counts is None or counts.tolist() == rc.tolist(), want
    loops, vertices, counts = dev_coverage(ctx, k, l, v, c, 12, loops_rows_out=0, vertex_rows_out=0)  # pointers with no rows are no tables
    assert counts.tolist() == rc.tolist()


def test_truncated_outputs_keep_the_full_prefix_sum(ctx):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    nl, nv = len(rl), len(rv)
    assert nl > 8 and nv > 8
    for lrows, vrows in ((0, nv), (1, nv), (nl - 1, nv), (nl, nv), (nl + 7, nv), (nl, 0), (nl, 1), (nl, nv - 1), (nl, nv + 7), (1, 1)):
        loops, vertices, counts = dev_coverage(ctx, k, l, v, c, 12, loops_rows_out=lrows, vertex_rows_out=vrows)
        assert counts.tolist() == rc.tolist(), (lrows, vrows)  # the full counts: that is how a caller sees truncation
        ml, mv = min(nl, lrows), min(nv, vrows)
        assert (loops[:ml] == rl[:ml]).all() and (loops[ml:] == POISON32).all(), (lrows, vrows)
        assert (vertices[:mv] == rv[:mv]).all() and (vertices[mv:] == POISON32).all(), (lrows, vrows)


def test_augmented_capacity(ctx):
    """aug_rows exactly n_aug is enough; one below is OVERFLOW: {n_loops, 0, 0, 4, n_aug, 0} and nothing else"""
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    n_aug = int(rc[4])
    assert n_aug > len(v)
    check_result((rl, rv, rc), dev_coverage(ctx, k, l, v, c, 12, aug_rows=n_aug))
    loops, vertices, counts = dev_coverage(ctx, k, l, v, c, 12, aug_rows=n_aug - 1)
    assert counts.tolist() == [len(l), 0, 0, _lib.COVERAGE_OVERFLOW, n_aug, 0]
    assert (loops == POISON32).all() and (vertices == POISON32).all()
    assert V.coverage(k, l, v, c, 12, aug_rows=n_aug - 1)[2].tolist() == counts.tolist()
    assert dev_coverage(ctx, k, l, v, c, 12, aug_rows=1)[2].tolist() == counts.tolist()


def test_status_bit_0_truncated_input(ctx):
    """input counts above the declared rows: {n_loops, 0, 0, 1, 0, 0} and nothing else"""
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    k, (l, v, c), _ = smooth_case()
    nl, nv = len(l), len(v)
    for lin, vin in ((nl - 1, nv), (nl, nv - 1), (1, 1), (0, nv), (nl, 0), (0, 0)):
        loops, vertices, counts = dev_coverage(ctx, k, l, v, c, 12, loops_rows_in=lin, vertex_rows_in=vin, loops_rows_out=nl, vertex_rows_out=nv)
        assert counts.tolist() == [nl, 0, 0, _lib.COVERAGE_TRUNCATED, 0, 0], (lin, vin)
        assert (loops == POISON32).all() and (vertices == POISON32).all(), (lin, vin)
        assert V.coverage(k, l, v, c, 12, loops_rows_in=lin, vertex_rows_in=vin)[2].tolist() == counts.tolist()
    assert dev_coverage(ctx, k, l, v, c, 12, loops_rows_in=nl, vertex_rows_in=nv)[2][3] == 0  # rows as large as the counts are enough


def test_status_bit_1_malformed_loops(ctx):
    """a diagonal edge, an id beyond the lattice, COUNT < 2, OFFSET + COUNT beyond the count: COUNT' = 0, the other loops as ever.
    No record here points outside the vertices the test itself allocated: the bad range ends inside the spare rows"""
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    k, (l, v, c), _ = smooth_case()
    nl, nv = len(l), len(v)
    for tol16 in (0, 12, 64):
        bad_l, bad_v = l.copy(), v.copy()
        bad_v[l[1, V.OFFSET] + 1] += 132        # one vertex a lattice row and a column away: two diagonal edges
        bad_v[l[3, V.OFFSET]] = 66 * 131 + 7    # an id beyond the (65 + 1) x (130 + 1) lattice
        bad_l[5, V.COUNT] = 1                   # too short
        bad_l[nl - 1, V.COUNT] += 3             # ends 3 beyond n_vertices (inside the spare rows)
        wrong = [1, 3, 5, nl - 1]
        ref = V.coverage(k, bad_l, bad_v, c, tol16)
        assert ref[2][3] == _lib.COVERAGE_MALFORMED and (ref[0][wrong, V.COUNT] == 0).all() and ref[2][2] >= 4
        check_result(ref, dev_coverage(ctx, k, bad_l, bad_v, c, tol16, spare=64), tol16)
        good = V.coverage(k, l, v, c, tol16)
        keep = np.ones(nl, bool)
        keep[wrong] = False
        assert (ref[0][keep][:, V.COUNT] == good[0][keep][:, V.COUNT]).all()  # the well-formed loops are simplified as ever
        for i in np.flatnonzero(keep).tolist():
            assert (ref[1][ref[0][i, 0]:ref[0][i, 0] + ref[0][i, 1]] == good[1][good[0][i, 0]:good[0][i, 0] + good[0][i, 1]]).all()


def test_calls_are_repeatable(ctx):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    k, (l, v, c), ref = smooth_case(16)
    first = dev_coverage(ctx, k, l, v, c, 16)
    again = dev_coverage(ctx, k, l, v, c, 16)
    k2 = R.noise(135, 241, 3, seed=9)
    other = dev_coverage(ctx, k2, *O.outline(k2), 16)  # another plane, a larger one, in between
    third = dev_coverage(ctx, k, l, v, c, 16)
    check_result(ref, first)
    for run in (again, third):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run, first))
    assert other[2].tolist() != ref[2].tolist()


def test_rules_and_error_codes(ctx):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    L, h = ctx.L, ctx.h
    k, (l, v, c), (rl, rv, rc) = smooth_case()
    d = Dev(ctx, plane=k.nbytes, lin=l.nbytes, vin=v.nbytes, cin=12, loops=l.nbytes, vertices=int(rc[4]) * 4, counts=24)
    try:
        d.put("plane", k)
        d.put("lin", l)
        d.put("vin", v)
        d.put("cin", c)
        P = d.ptr
        call = lambda hh=65, ww=130, tol=12, eb=1, fl=0, sk=0, pl=P["plane"], li=P["lin"], ve=P["vin"], n=P["cin"], lo=P["loops"], vo=P["vertices"], co=P["counts"], ar=0: \
            L.infur_coverage_dev(h, pl, eb, hh, ww, fl, sk, li, len(l), ve, len(v), n, tol, ar, lo, len(l), vo, int(rc[4]), co)  # noqa: E731
        assert call(ww=0) == call(ww=8192) == call(hh=0) == call(hh=8192) == _lib.E_INVALID_ARG
        assert call(tol=65536) == _lib.E_INVALID_ARG and "tol16" in ctx.last_error()
        assert call(fl=2) == _lib.E_INVALID_ARG and call(fl=4) == _lib.E_INVALID_ARG and "flags" in ctx.last_error()  # connectivity is no input
        assert call(fl=1, sk=256) == _lib.E_INVALID_ARG and call(eb=2) == _lib.E_INVALID_ARG
        assert call(lo=None, vo=None, co=None) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()
        assert call(pl=None) == call(n=None) == call(li=None) == call(ve=None) == _lib.E_INVALID_ARG
        assert call(ar=0xFFFFFFFF) == _lib.E_INVALID_ARG
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("loops", "vertices", "counts"))  # no output is touched by a rejected call
        assert call() == _lib.OK
        ctx.synchronize()
        got = (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32))
        check_result((rl, rv, rc), got)
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    lo, vo, co = np.full((len(l), 4), 9, np.uint32), np.full(int(rc[4]), 9, np.uint32), np.full(6, 77, np.uint32)
    host = lambda ww=130, tol=12, fl=0, pl=k.ctypes.data, li=l.ctypes.data, n=c.ctypes.data, lout=lo.ctypes.data, vout=vo.ctypes.data, cout=co.ctypes.data: \
        L.infur_coverage(h, pl, 1, 65, ww, fl, 0, li, len(l), v.ctypes.data, len(v), n, tol, 0, lout, len(l), vout, len(vo), cout)  # noqa: E731
    assert host(ww=0) == host(ww=8192) == host(tol=65536) == host(fl=2) == host(pl=None) == host(li=None) == host(n=None) == _lib.E_INVALID_ARG
    assert host(lout=None, vout=None, cout=None) == _lib.E_INVALID_ARG
    assert (lo == 9).all() and (vo == 9).all() and (co == 77).all()
    assert host() == _lib.OK and co.tolist() == rc.tolist() and (lo == rl).all() and (vo[:len(rv)] == rv).all() and (vo[len(rv):] == 9).all()
    with pytest.raises(Exception):
        Coverage(ctx).control(SimplifyCmd.Tol16(65536))


# --------------------------------------------------------------------------- #
# 3. the fused frame path
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_frame_outlines_then_coverage(ctx, model, decode):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    fp = FramePath(ctx)
    for h, w in ((48, 64), (61, 97)):
        frame = W.synth_frame(h, w, index=h)
        s = fp.advance_segments(frame, 1.0, decode)
        o = fp.advance_outlines(frame, 1.0, decode, loops_rows=h * w, vertex_rows=4 * h * w)
        assert (o.loops == O.outline(s.klass)[0]).all()
        for tol16 in (11, 16):
            out = CoverageOut(loops_rows=h * w, vertex_rows=5 * h * w + h + w + 1)
            Coverage(ctx, tol16).advance((s.klass, o.loops, o.vertices, o.counts[:2], None), out)
            rl, rv, rc = V.coverage(s.klass, o.loops, o.vertices, o.counts, tol16)
            assert (out.loops == rl).all() and (out.vertices == rv).all()
            r = fp.advance_coverage(frame, 1.0, decode, tol16, loops_rows=len(rl) + 1, vertex_rows=len(rv) + 1, want_scaled=True)
            assert list(r.counts) == rc.tolist() and (r.loops == rl).all() and (r.vertices == rv).all() and r.shape == (h, w), (h, w, tol16)
            assert r.stats.tobytes() == s.stats.tobytes() and r.scaled.shape == (h, w, 3)
            V.check_invariants(s.klass, r.loops, r.vertices, np.array(r.counts))
        # skip, 8-connectivity, an edge capacity that is just enough, truncated tables; no statistics
        skip_value = int(s.klass[0, 0])
        sl, sv, sc = O.outline(s.klass, SKIP | CONN8, skip_value)
        ql, qv, qc = V.coverage(s.klass, sl, sv, sc, 16, V.SKIP, skip_value)
        q = fp.advance_coverage(frame, 1.0, decode, 16, skip=skip_value, connectivity=8, max_edges=int(sc[2]), loops_rows=2, vertex_rows=3, want_stats=False)
        assert list(q.counts) == qc.tolist() and q.stats is None and (q.loops == ql[:2]).all() and (q.vertices == qv[:3]).all()
        q = fp.advance_coverage(frame, 1.0, decode, 16, max_edges=int(o.counts[2]) - 1)  # more edges than the capacity: nothing
        assert list(q.counts) == [0] * 6 and len(q.loops) == 0 and len(q.vertices) == 0


def test_fused_device_call_and_its_rules(ctx, model):
    assert ctx.L.infur_features() & _lib.FEATURE_COVERAGE
    L, h = ctx.L, ctx.h
    hh, ww = 61, 97
    frame = W.synth_frame(hh, ww, index=2)
    s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
    ref = V.coverage(s.klass, *O.outline(s.klass), 12)
    rl, rv, rc = ref
    k = s.stats.shape[0]
    d = Dev(ctx, bgr=frame.nbytes, loops=(len(rl) + 2) * 16, vertices=(len(rv) + 2) * 4, counts=24, stats=k * 64)
    try:
        d.put("bgr", frame)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        P = d.ptr
        call = lambda tol=12, flags=0, skip=0, mode=0, decode=SOFTMAX, lo=P["loops"], ve=P["vertices"], co=P["counts"], st=P["stats"]: L.infur_frame_coverage_dev(  # noqa: E731
            h, P["bgr"], ww, hh, 1.0, mode, decode, flags, skip, 0, tol, lo, len(rl) + 2, ve, len(rv) + 2, co, st, k, None, C.byref(ow), C.byref(oh))
        assert call(tol=65536) == call(flags=4) == call(flags=SKIP, skip=256) == call(mode=2) == call(decode=2) == _lib.E_INVALID_ARG
        assert call(lo=None, ve=None, co=None) == _lib.E_INVALID_ARG
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("loops", "vertices", "counts"))
        for stats in (True, False):
            d.poison("loops", "vertices", "counts", "stats")
            ctx.check(call(st=P["stats"] if stats else None))
            ctx.synchronize()
            assert (ow.value, oh.value) == (ww, hh)
            check_result(ref, (d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32)))
            assert d.get("stats").tobytes() == s.stats.tobytes() if stats else (d.get("stats") == POISON).all()
    finally:
        d.free()


# --------------------------------------------------------------------------- #
# 4. the command line
# --------------------------------------------------------------------------- #
def test_cli_outlines_shared(tmp_path):
    """--outlines-shared: the fused call on the class plane, the host class plane beside it, and the label plane Regions left"""
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip),
            "--outlines-shared"]

    def cli(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout + r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]

    recs = cli("--labels-out", str(tmp_path / "klass.u8"), "--outlines-out", str(tmp_path / "klass.outl"), "--outlines-tolerance", "1")
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    fused = cli("--outlines-out", str(tmp_path / "fused.outl"), "--connectivity", "4", "--outlines-tolerance", "1")
    for i, ((counts, loops, verts), (fc, fl, fv)) in enumerate(zip(TO.read_outlines_file(tmp_path / "klass.outl", 2), TO.read_outlines_file(tmp_path / "fused.outl", 2))):
        rl, rv, rc = V.coverage(klass[i], *O.outline(klass[i], CONN8), 16)  # (8-connectivity is the command line's default)
        assert recs[i]["n_loops"] == rc[0] and recs[i]["n_degenerate"] == rc[2] and counts.tolist() == rc[:3].tolist()
        assert (loops == rl).all() and (verts == rv).all()
        V.check_invariants(klass[i], loops, verts, rc)
        ql, qv, qc = V.coverage(klass[i], *O.outline(klass[i]), 16)
        assert fc.tolist() == qc[:3].tolist() and (fl == ql).all() and (fv == qv).all() and fused[i]["classes"] == recs[i]["classes"]
    lines = cli("--regions", "--min-pixels", "3", "--skip-background", "--outlines-skip", str(NONE), "--max-regions", str(96 * 128), "--regions-out",
                str(tmp_path / "labels.u32"), "--outlines-out", str(tmp_path / "labels.outl"), "--outlines-tolerance", "0.75")
    dense = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    for i, (counts, loops, verts) in enumerate(TO.read_outlines_file(tmp_path / "labels.outl", 2)):
        rl, rv, rc = V.coverage(dense[i], *O.outline(dense[i], SKIP | CONN8, NONE), 12, V.SKIP, NONE)
        assert lines[i]["n_loops"] == rc[0] and counts.tolist() == rc[:3].tolist() and (loops == rl).all() and (verts == rv).all()
        assert sorted(outlines_by_value(loops, verts, 128)) == list(range(len(lines[i]["regions"])))
