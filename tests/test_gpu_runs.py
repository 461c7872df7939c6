"""Runs on the GPU: records, per-row index and count of ``infur_runs*`` and of the fused ``infur_frame_runs*`` against
tests/runs_ref.py.  Everything is an integer and a function of the plane alone, so every comparison is ``==`` on whole arrays.
Every output buffer is filled with a poison byte first: what a call must leave alone still holds it afterwards, and what it must
write owes nothing to an initialisation."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Context, FramePath, Model, ModelCmd, Runs, RunsCmd, RunsOut, runs_by_value, runs_decode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
SKIP = _lib.RUNS_SKIP
NONE = 0xFFFFFFFF
GUARD = 64
POISON = 0xA5
POISON32 = 0xA5A5A5A5


class Dev:
    """device buffers with GUARD poisoned bytes behind each; the whole buffer is poisoned when it is made"""

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


def dev_runs(ctx, plane, flags=0, skip_value=0, rows=0, want=("runs", "row_start", "n")):
    """infur_runs_dev on poisoned device buffers -> (runs [rows, 3] u32 as the buffer holds it, row_start [h + 1] u32, n), None
    for what was not wanted (and that buffer is checked to be untouched)"""
    h, w = plane.shape
    d = Dev(ctx, plane=plane.nbytes, runs=rows * 12, row_start=(h + 1) * 4, n=4)
    try:
        d.put("plane", plane)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_runs_dev(ctx.h, d.ptr["plane"], plane.dtype.itemsize, h, w, flags, skip_value, p("runs"), rows, p("row_start"), p("n")))
        ctx.synchronize()
        runs, row_start, n = d.get("runs").view(np.uint32).reshape(rows, 3), d.get("row_start").view(np.uint32), d.get("n").view(np.uint32)
        assert d.get("plane").tobytes() == plane.tobytes()  # the input is an input
        for name, got in (("runs", runs), ("row_start", row_start), ("n", n)):
            if name not in want:
                assert (got.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return (runs if "runs" in want else None, row_start if "row_start" in want else None, int(n[0]) if "n" in want else None)
    finally:
        d.free()


def check_against_reference(ctx, plane, flags=0, skip_value=0, name="", spare=7):
    rr, rrs, rn = U.encode(plane, flags, skip_value)
    runs, row_start, n = dev_runs(ctx, plane, flags, skip_value, rows=rn + spare)
    print(f"{name} {plane.shape[0]}x{plane.shape[1]} {plane.dtype} flags {flags} skip {skip_value}: {rn} runs")
    assert n == rn, (name, plane.shape, n, rn)
    assert (row_start == rrs).all(), (name, plane.shape)
    assert (runs[:rn] == rr).all(), (name, plane.shape)
    assert (runs[rn:] == POISON32).all(), "records at or beyond n were written"
    return rr, rrs, rn


def families(h, w):
    yield "smooth", R.smooth(h, w, seed=h + w)
    yield "noise2", R.noise(h, w, 2, seed=w)
    yield "noise21", R.noise(h, w, 21, seed=h)
    yield "single", R.single(h, w)
    yield "vstripes", R.stripes(h, w, vertical=True)
    yield "hstripes", R.stripes(h, w, vertical=False)
    yield "checkerboard", R.checkerboard(h, w)
    yield "staircase", R.staircase(h, w)


def as_elem(klass, elem_bytes):
    return klass if elem_bytes == 1 else U.as_u32(klass)


SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (135, 241))


# --------------------------------------------------------------------------- #
# 1. infur_runs_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_families_equal_the_reference(ctx, elem_bytes):
    assert ctx.L.infur_features() & _lib.FEATURE_RUNS  # (the first line: fails on a library without the feature)
    counts = {}
    for h, w in SHAPES:
        for name, k in families(h, w):
            plane = as_elem(k, elem_bytes)
            counts[(name, h, w)] = check_against_reference(ctx, plane, name=name)[2]
            # skip on: the value of the first pixel (a run at index 0 goes), of the last pixel, and one the u32 table maps to NONE
            for skip_value in sorted({int(plane[0, 0]), int(plane[-1, -1]), int(as_elem(np.zeros((1, 1), np.uint8), elem_bytes)[0, 0])}):
                rn = check_against_reference(ctx, plane, SKIP, skip_value, name=name)[2]
                assert (rn < counts[(name, h, w)]) == bool((plane == skip_value).any())
    # what the families are for
    assert counts[("single", 135, 241)] == 135 == counts[("hstripes", 135, 241)]  # a run never continues into the next row
    assert counts[("checkerboard", 135, 241)] == 135 * 241 == counts[("vstripes", 135, 241)]
    assert counts[("single", 1, 1)] == 1 and counts[("checkerboard", 5, 1)] == 5 and counts[("single", 3, 64)] == 3
    if elem_bytes == 4:
        t = U.u32_table()
        assert t[0] == NONE and (t > (1 << 24)).sum() > 200  # the u32 planes do hold 0xFFFFFFFF and values a float would round


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_runs_that_span_workgroups_and_rows_of_one_pixel(ctx, elem_bytes):
    # one run whose head and tail lie in different workgroups (1024 pixels each)
    rr, rrs, rn = check_against_reference(ctx, as_elem(R.single(1, 3000), elem_bytes), name="single")
    assert rn == 1 and rr.tolist() == [[0, 3000, int(as_elem(R.single(1, 1), elem_bytes)[0, 0])]] and rrs.tolist() == [0, 1]
    # every pixel is a run and a row
    rr, rrs, rn = check_against_reference(ctx, as_elem(R.single(3000, 1), elem_bytes), name="single")
    assert rn == 3000 and (rrs == np.arange(3001)).all() and (rr[:, U.END] - rr[:, U.START] == 1).all()
    check_against_reference(ctx, as_elem(R.noise(1, 3000, 2, seed=4), elem_bytes), SKIP, int(as_elem(np.ones((1, 1), np.uint8), elem_bytes)[0, 0]), name="noise2")


@pytest.mark.parametrize("name", ["single", "checkerboard"])
def test_more_than_1024_block_sums(ctx, name):
    """1100 x 1000 pixels are 1075 workgroups: the scan of the block sums takes a second pass"""
    k = R.single(1100, 1000) if name == "single" else R.checkerboard(1100, 1000)
    rn = check_against_reference(ctx, k, name=name)[2]
    assert rn == (1100 if name == "single" else 1100 * 1000)
    if name == "checkerboard":
        assert check_against_reference(ctx, U.as_u32(k), SKIP, int(U.u32_table()[1]), name=name)[2] == 550 * 1000


def test_1080p_smooth_plane(ctx):
    k = R.smooth(1080, 1920)
    rr, _, rn = check_against_reference(ctx, k, name="smooth")
    assert 4 * rn * 12 < k.size * 4  # blobs 24 pixels across: the records are under a quarter of the bytes of a u32 plane
    check_against_reference(ctx, U.as_u32(k), SKIP, NONE, name="smooth as u32")  # (the table maps class 0 to 0xFFFFFFFF)


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_truncation(ctx, elem_bytes):
    for name, k in (("smooth", R.smooth(135, 241)), ("noise21", R.noise(33, 63, 21)), ("checkerboard", R.checkerboard(7, 65))):
        plane = as_elem(k, elem_bytes)
        for flags, skip_value in ((0, 0), (SKIP, int(plane[3, 3]))):
            rr, rrs, rn = U.encode(plane, flags, skip_value)
            assert rn > 8
            for rows in (0, 1, rn - 1, rn, rn + 7):
                runs, row_start, n = dev_runs(ctx, plane, flags, skip_value, rows=rows)
                m = min(rn, rows)
                assert n == rn, (name, rows)  # the full count: that is how a caller sees truncation
                assert (row_start == rrs).all(), (name, rows)  # whatever runs_rows is
                assert (runs[:m] == rr[:m]).all() and (runs[m:] == POISON32).all(), (name, rows)


def test_calls_are_repeatable_and_contexts_agree(ctx):
    k = R.noise(135, 241, 3, seed=9)
    rn = U.encode(k)[2]
    first = dev_runs(ctx, k, rows=rn)
    again = dev_runs(ctx, k, rows=rn)
    other = dev_runs(ctx, R.smooth(270, 480), rows=rn)  # another plane, a larger one, in between
    third = dev_runs(ctx, k, rows=rn)
    with Context(device=0) as c2:
        second_ctx = dev_runs(c2, k, rows=rn)
    for run in (again, third, second_ctx):
        assert run[2] == first[2] == rn and run[0].tobytes() == first[0].tobytes() and run[1].tobytes() == first[1].tobytes()
    assert other[2] != rn


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_each_output_alone_equals_all_together(ctx, elem_bytes):
    for k in (R.smooth(135, 241), R.noise(7, 65, 3), R.noise(1, 5, 3)):
        plane = as_elem(k, elem_bytes)
        skip_value = int(plane[0, 0])
        rr, rrs, rn = U.encode(plane, SKIP, skip_value)
        for want in (("runs",), ("row_start",), ("n",), ("runs", "n"), ("row_start", "n"), ("runs", "row_start")):
            runs, row_start, n = dev_runs(ctx, plane, SKIP, skip_value, rows=rn, want=want)
            assert runs is None or (runs == rr).all(), want
            assert row_start is None or (row_start == rrs).all(), want
            assert n is None or n == rn, want
        # a records pointer with no rows is no table
        runs, row_start, n = dev_runs(ctx, plane, SKIP, skip_value, rows=0)
        assert (row_start == rrs).all() and n == rn


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    k = R.noise(6, 7, 3)
    d = Dev(ctx, plane=42 * 4, runs=12 * 50, row_start=8 * 4, n=4)
    try:
        d.put("plane", U.as_u32(k))
        P = d.ptr
        call = lambda elem=4, flags=0, skip=0, hh=6, ww=7, pl=P["plane"], runs=P["runs"], rs=P["row_start"], n=P["n"]: L.infur_runs_dev(  # noqa: E731
            h, pl, elem, hh, ww, flags, skip, runs, 50, rs, n)
        for elem in (0, 2, 3, 8):
            assert call(elem=elem) == _lib.E_INVALID_ARG
        assert call(flags=2) == _lib.E_INVALID_ARG and call(flags=3) == _lib.E_INVALID_ARG  # an unknown flag bit
        assert call(elem=1, flags=SKIP, skip=256) == _lib.E_INVALID_ARG and call(elem=1, skip=256) == _lib.E_INVALID_ARG
        assert call(runs=None, rs=None, n=None) == _lib.E_INVALID_ARG  # all outputs NULL
        assert "no output wanted" in ctx.last_error()
        assert L.infur_runs_dev(h, P["plane"], 4, 6, 7, 0, 0, P["runs"], 0, None, None) == _lib.E_INVALID_ARG  # records without rows: not wanted
        assert call(pl=None) == _lib.E_INVALID_ARG and "no plane pointer" in ctx.last_error()
        assert call(hh=65536, ww=65536) == _lib.E_INVALID_ARG and call(hh=0xFFFFFFFF, ww=1) == _lib.E_INVALID_ARG  # h*w >= 2^32 - 1
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("runs", "row_start", "n"))  # no output is touched by a rejected call
        # an empty plane: n_runs = 0, row_start[0..h] = 0 and nothing else
        for hh, ww in ((0, 7), (6, 0), (0, 0)):
            d.poison("n", "row_start")
            assert call(hh=hh, ww=ww, pl=None) == _lib.OK
            ctx.synchronize()
            rs = d.get("row_start").view(np.uint32)
            assert d.get("n").view(np.uint32)[0] == 0 and (rs[:hh + 1] == 0).all() and (rs[hh + 1:] == POISON32).all()
            assert (d.get("runs") == POISON).all()
        assert call(hh=0, n=None) == _lib.OK and call(skip=256, flags=SKIP) == _lib.OK  # (a u32 plane may skip any u32)
        d.poison("n")
        assert call() == _lib.OK
        ctx.synchronize()
        assert d.get("n").view(np.uint32)[0] == U.encode(U.as_u32(k))[2]
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    n = C.c_uint32(77)
    runs = np.full((50, 3), 9, np.uint32)
    rs = np.full(8, 9, np.uint32)
    host = lambda elem=1, flags=0, skip=0, hh=6, ww=7, pl=k.ctypes.data, r=runs.ctypes.data, s=rs.ctypes.data, c=C.addressof(n): L.infur_runs(  # noqa: E731
        h, pl, elem, hh, ww, flags, skip, r, 50, s, c)
    assert host(elem=2) == host(flags=4) == host(skip=300) == host(pl=None) == host(r=None, s=None, c=None) == _lib.E_INVALID_ARG
    assert host(hh=65536, ww=65536) == _lib.E_INVALID_ARG
    assert n.value == 77 and (runs == 9).all() and (rs == 9).all()
    assert host(hh=0) == _lib.OK and n.value == 0 and rs.tolist() == [0] + [9] * 7 and (runs == 9).all()
    rs[:] = 9
    assert host(ww=0) == _lib.OK and n.value == 0 and rs.tolist() == [0] * 7 + [9] and (runs == 9).all()
    with pytest.raises(Exception):
        Runs(ctx).control(RunsCmd.Skip(-1))


@pytest.mark.parametrize("elem_bytes", [1, 4])
def test_host_pointer_call_and_processor(ctx, elem_bytes):
    proc = Runs(ctx)
    assert proc.is_dirty()
    for k in (R.smooth(135, 241), R.noise(33, 63, 21), R.stripes(7, 65)):
        plane = as_elem(k, elem_bytes)
        hh, ww = plane.shape
        rr, rrs, rn = U.encode(plane)
        dr, drs, dn = dev_runs(ctx, plane, rows=rn)
        out = RunsOut(runs_rows=rn + 5)
        proc.control(RunsCmd.Skip(None)).advance(plane, out)
        assert not proc.is_dirty() and out.n == rn == dn and out.runs.shape == (rn, 3)
        assert (out.runs == dr).all() and (out.row_start == drs).all() and (out.runs == rr).all() and (out.row_start == rrs).all()
        assert (runs_decode(out.runs, out.n, hh, ww, dtype=plane.dtype) == plane).all()
        by = runs_by_value(out.runs, out.n)
        assert sorted(by) == np.unique(plane).tolist() and sum(int((v[:, 1] - v[:, 0]).sum()) for v in by.values()) == plane.size
        # the caller's records beyond n, and beyond runs_rows, are left alone
        runs = np.full((rn + 2, 3), 7, np.uint32)
        rs = np.full(hh + 1, 7, np.uint32)
        n = C.c_uint32(0)
        ctx.check(ctx.L.infur_runs(ctx.h, plane.ctypes.data, elem_bytes, hh, ww, 0, 0, runs.ctypes.data, rn + 2, rs.ctypes.data, C.addressof(n)))
        assert n.value == rn and (runs[:rn] == rr).all() and (runs[rn:] == 7).all() and (rs == rrs).all()
        runs[:] = 7
        ctx.check(ctx.L.infur_runs(ctx.h, plane.ctypes.data, elem_bytes, hh, ww, 0, 0, runs.ctypes.data, 1, None, C.addressof(n)))
        assert n.value == rn and (runs[0] == rr[0]).all() and (runs[1:] == 7).all()
        # skip, through the processor
        skip_value = int(plane[hh // 2, ww // 2])
        sr, srs, sn = U.encode(plane, SKIP, skip_value)
        out = RunsOut(runs_rows=2, want_row_start=False)
        proc.control(RunsCmd.Skip(skip_value))
        assert proc.is_dirty()
        proc.advance(plane, out)
        assert out.n == sn and out.row_start is None and (out.runs == sr[:2]).all()


def test_composition_with_regions_on_the_device(ctx):
    """infur_regions_dev, then infur_runs_dev on the label plane it left on the device: per-object runs, no dense plane to the host"""
    k = R.smooth(135, 241)
    h, w = k.shape
    flags, min_pixels = _lib.REGIONS_SKIP_BACKGROUND, 20
    labels = np.empty((h, w), np.uint32)
    n_reg = C.c_uint32(0)
    ctx.check(ctx.L.infur_regions(ctx.h, k.ctypes.data, None, h, w, 8, min_pixels, flags, labels.ctypes.data, None, 0, C.addressof(n_reg)))
    assert (labels == NONE).any() and n_reg.value > 3
    rr, rrs, rn = U.encode(labels, SKIP, NONE)
    d = Dev(ctx, klass=h * w, labels=h * w * 4, runs=(rn + 3) * 12, row_start=(h + 1) * 4, n=4)
    try:
        d.put("klass", k)
        P = d.ptr
        ctx.check(ctx.L.infur_regions_dev(ctx.h, P["klass"], None, h, w, 8, min_pixels, flags, P["labels"], None, 0, None))
        ctx.check(ctx.L.infur_runs_dev(ctx.h, P["labels"], 4, h, w, SKIP, NONE, P["runs"], rn + 3, P["row_start"], P["n"]))
        ctx.synchronize()
        runs = d.get("runs").view(np.uint32).reshape(rn + 3, 3)
        assert d.get("n").view(np.uint32)[0] == rn and (d.get("row_start").view(np.uint32) == rrs).all()
        assert (runs[:rn] == rr).all() and (runs[rn:] == POISON32).all()
        assert (d.get("labels").view(np.uint32).reshape(h, w) == labels).all()
        by = runs_by_value(runs, rn)  # one object's mask is its runs
        assert sorted(by) == list(range(n_reg.value))
        assert all(int((v[:, 1] - v[:, 0]).sum()) == int((labels == i).sum()) for i, v in by.items())
    finally:
        d.free()


# --------------------------------------------------------------------------- #
# 2. the fused frame path
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_segments_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    for (h, w), factor in (((61, 97), 1.0), ((120, 160), 1.0), ((120, 160), 0.5)):
        frame = W.synth_frame(h, w, index=h)
        s = fp.advance_segments(frame, factor, decode)
        oh, ow = s.klass.shape
        rr, rrs, rn = U.encode(s.klass)
        r = fp.advance_runs(frame, factor, decode, runs_rows=rn + 1, want_scaled=True)
        assert r.n == rn and (r.runs == rr).all() and (r.row_start == rrs).all(), (h, w, factor)
        assert r.stats.tobytes() == s.stats.tobytes()  # captions come with the mask
        assert r.scaled.shape == (oh, ow, 3)
        assert (runs_decode(r.runs, r.n, oh, ow) == s.klass).all()
        lo, _ = model.lowres()  # infur_model_read_lowres still works afterwards
        assert lo.size > 0 and np.isfinite(lo).all()
        # skip and a truncated table; no statistics, no row index
        skip_value = int(s.klass[0, 0])
        sr, srs, sn = U.encode(s.klass, SKIP, skip_value)
        q = fp.advance_runs(frame, factor, decode, skip=skip_value, runs_rows=2, want_row_start=False, want_stats=False)
        assert q.n == sn and q.row_start is None and q.stats is None and (q.runs == sr[:2]).all()


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    for hh, ww in ((52, 100), (50, 99)):
        frame = W.synth_frame(hh, ww, index=2)
        s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
        rr, rrs, rn = U.encode(s.klass)
        k = s.stats.shape[0]
        d = Dev(ctx, bgr=frame.nbytes, runs=(rn + 2) * 12, row_start=(hh + 1) * 4, n=4, stats=k * 64)
        try:
            d.put("bgr", frame)
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            P = d.ptr
            for stats in (True, False):
                d.poison("runs", "row_start", "n", "stats")
                ctx.check(L.infur_frame_runs_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 0, 0, P["runs"], rn + 2, P["row_start"], hh + 1, P["n"],
                                                 P["stats"] if stats else None, k, None, C.byref(ow), C.byref(oh)))
                ctx.synchronize()
                assert (ow.value, oh.value) == (ww, hh)
                runs = d.get("runs").view(np.uint32).reshape(rn + 2, 3)
                assert d.get("n").view(np.uint32)[0] == rn and (d.get("row_start").view(np.uint32) == rrs).all()
                assert (runs[:rn] == rr).all() and (runs[rn:] == POISON32).all()
                if stats:
                    assert d.get("stats").tobytes() == s.stats.tobytes()
                else:
                    assert (d.get("stats") == POISON).all()
        finally:
            d.free()


def test_fused_rules_and_error_codes(ctx, model):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    runs = np.full((48 * 64, 3), 9, np.uint32)
    rs = np.full(49, 9, np.uint32)
    stats = np.zeros((21, 8), np.uint64)
    n, ow, oh = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(lib=L, handle=h, decode=0, flags=0, skip=0, r=runs, row_start=rs, rs_rows=49, count=n, st=stats, st_cap=21, mode=0, factor=1.0, scaled=None):
        return lib.infur_frame_runs(handle, p(frame), 64, 48, factor, mode, decode, flags, skip, p(r), 48 * 64, p(row_start), rs_rows,
                                    C.addressof(count) if count is not None else None, p(st), st_cap, p(scaled), C.byref(ow), C.byref(oh))

    klass = FramePath(ctx).advance_segments(frame, 1.0, RAW).klass
    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48) and n.value == U.encode(klass)[2] and (rs == U.encode(klass)[1]).all()
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) == _lib.E_INVALID_ARG
    assert call(flags=2) == _lib.E_INVALID_ARG and call(flags=SKIP, skip=256) == _lib.E_INVALID_ARG
    assert call(r=None, row_start=None, count=None) == _lib.E_INVALID_ARG
    assert call(rs_rows=48) == _lib.E_CAPACITY  # row_start_rows = oh
    assert call(row_start=None, rs_rows=0) == _lib.OK  # no index wanted: its capacity does not matter
    assert call(st_cap=20) == _lib.E_CAPACITY and call(st=None, st_cap=0) == _lib.OK
    assert call(factor=-1.0) == _lib.E_INVALID_SCALE
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_runs(frame, 0.5, RAW, want_scaled=True)
        assert r.runs is None and r.row_start is None and r.n is None and r.stats is None and r.scaled.shape == (24, 32, 3)
        assert (r.scaled == FramePath(c).advance_segments(frame, 0.5, RAW, want_scaled=True).scaled).all()
        runs[:] = 9
        n.value = 77
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED
        want_scaled = FramePath(c).advance_segments(frame, 1.0, RAW, want_scaled=True).scaled
        assert (scaled == want_scaled).all() and (runs == 9).all() and n.value == 77
        scaled[:] = 0  # a row index that is too short changes nothing about that: capacities are checked once a model is loaded
        assert call(lib=c.L, handle=c.h, scaled=scaled, rs_rows=3) == _lib.E_MODEL_NOT_LOADED and (scaled == want_scaled).all()


def test_runs_calls_leave_the_cached_graphs_alone(blob50):
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
        for it in range(8):
            fr = frames[it % 4]
            args = (fr, 1.0, SOFTMAX if it & 1 else RAW, 0 if it & 2 else None)
            s = fg.advance_runs(*args, want_stats=bool(it & 4))
            e = fe.advance_runs(*args)
            assert s.n == e.n and (s.runs == e.runs).all() and (s.row_start == e.row_start).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a runs call caused a capture"
        assert cached1 >= cached0, "a runs call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the runs calls were not replayed"


# --------------------------------------------------------------------------- #
# 3. the command line
# --------------------------------------------------------------------------- #
def read_runs_file(path, frames):
    """-> [(n, records [n, 3])] of a --runs-out file, which must hold exactly `frames` frames"""
    words = np.frombuffer(open(path, "rb").read(), np.uint32)
    out, at = [], 0
    for _ in range(frames):
        n = int(words[at])
        out.append((n, words[at + 1:at + 1 + 3 * n].reshape(n, 3)))
        at += 1 + 3 * n
    assert at == len(words)
    return out


def test_cli_round_trip(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip)]

    def cli(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]

    # the class plane beside its records: the records decode to the bytes of --labels-out
    recs = cli("--labels-out", str(tmp_path / "klass.u8"), "--runs-out", str(tmp_path / "klass.runs"))
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    got = read_runs_file(tmp_path / "klass.runs", 2)
    for i, (n, runs) in enumerate(got):
        assert sorted(recs[i]) == ["classes", "frame", "height", "n_runs", "width"] and recs[i]["n_runs"] == n == U.encode(klass[i])[2]
        assert runs_decode(runs, n, 96, 128).tobytes() == klass[i].tobytes()
    # the fused call (no dense plane asked for), without the background class: the same records less those of class 0, the same captions
    fused = cli("--runs-out", str(tmp_path / "fused.runs"), "--runs-skip", "0")
    for i, (n, runs) in enumerate(read_runs_file(tmp_path / "fused.runs", 2)):
        assert fused[i]["n_runs"] == n and (runs == U.encode(klass[i], SKIP, 0)[0]).all() and fused[i]["classes"] == recs[i]["classes"]
    # per-track runs from the plane Tracks left on the device, beside both dense planes
    common = ("--tracks", "--min-pixels", "3", "--skip-background", "--runs-skip", str(NONE), "--max-regions", str(96 * 128))
    lines = cli(*common, "--regions-out", str(tmp_path / "labels.u32"), "--tracks-out", str(tmp_path / "tracks.u32"),
                "--runs-out", str(tmp_path / "tracks.runs"), "--runs-plane", "tracks")
    # per-object runs with no dense plane written out: the label plane never leaves the device, the records are those of the
    # plane the run above wrote
    alone = cli(*common, "--runs-out", str(tmp_path / "labels.runs"), "--runs-plane", "labels")
    for out, recs_file, js in (("tracks.u32", "tracks.runs", lines), ("labels.u32", "labels.runs", alone)):
        dense = np.frombuffer((tmp_path / out).read_bytes(), np.uint32).reshape(2, 96, 128)
        for i, (n, runs) in enumerate(read_runs_file(tmp_path / recs_file, 2)):
            assert js[i]["n_runs"] == n and (runs == U.encode(dense[i], SKIP, NONE)[0]).all()
            assert runs_decode(runs, n, 96, 128, fill=NONE, dtype=np.uint32).tobytes() == dense[i].tobytes()
