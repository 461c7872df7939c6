"""Regions on the GPU: label plane, region table and region count of ``infur_regions*`` and of the fused
``infur_frame_regions*`` against tests/regions_ref.py.  Everything is an integer and the numbering is canonical (ascending first
pixel), so every comparison is ``==`` on whole arrays, for both connectivities."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import (Context, FramePath, InfurError, Model, ModelCmd, Regions, RegionsCmd, RegionsOut, class_summary,
                                  region_summary)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import segments_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
NONE = int(R.NONE)
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


def dev_regions(ctx, klass, conf, conn, min_pixels=0, flags=0, table_rows=0, want=("labels", "table", "n")):
    """infur_regions_dev on poisoned device buffers -> (labels [h, w] u32, table [table_rows, 10] u64 as the buffer holds it, n),
    None for what was not wanted"""
    h, w = klass.shape
    d = Dev(ctx, klass=h * w, conf=h * w, labels=h * w * 4, table=table_rows * 80, n=4)
    try:
        d.put("klass", klass)
        if conf is not None:
            d.put("conf", conf)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_regions_dev(ctx.h, d.ptr["klass"], d.ptr["conf"] if conf is not None else None, h, w, conn, min_pixels, flags,
                                          p("labels"), p("table"), table_rows, p("n")))
        ctx.synchronize()
        labels, table, n = d.get("labels").view(np.uint32).reshape(h, w), d.get("table").view(np.uint64).reshape(table_rows, 10), d.get("n")
        assert (d.get("klass") == klass.ravel()).all()  # the inputs are inputs
        for name, got in (("labels", labels), ("table", table), ("n", n)):
            if name not in want:
                assert (got.view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
        return (labels if "labels" in want else None, table if "table" in want else None, int(n.view(np.uint32)[0]) if "n" in want else None)
    finally:
        d.free()


def check_against_reference(ctx, klass, conn, min_pixels=0, flags=0, name="", spare_rows=3):
    conf = R.conf_for(klass, seed=klass.shape[1])
    rl, rt, rn = R.label(klass, conf, conn, min_pixels, flags)
    labels, table, n = dev_regions(ctx, klass, conf, conn, min_pixels, flags, table_rows=rn + spare_rows)
    print(f"{name} {klass.shape[0]}x{klass.shape[1]} connectivity {conn}: {rn} regions")
    assert n == rn, (name, conn, n, rn)
    assert (labels == rl).all(), (name, conn)
    assert (table[:rn] == rt).all(), (name, conn)
    assert (table[rn:].view(np.uint8) == POISON).all(), "rows at or beyond n were written"
    return rl, rt, rn


def small_families():
    yield "smooth", R.smooth(33, 47)
    yield "smooth", R.smooth(270, 480)
    yield "noise21", R.noise(270, 480, 21)
    yield "noise3", R.noise(270, 480, 3)
    yield "noise3", R.noise(65, 130, 3)
    yield "single", R.single(65, 130)
    yield "serpentine", R.serpentine(65, 130)
    yield "serpentine", R.serpentine(270, 480)
    yield "spiral", R.spiral(65, 130, arms=2)
    yield "spiral", R.spiral(270, 480, arms=2)
    yield "vstripes", R.stripes(65, 130, vertical=True)
    yield "hstripes", R.stripes(65, 130, vertical=False)
    yield "staircase", R.staircase(65, 130)
    yield "staircase", R.staircase(270, 480, period=2)
    yield "checkerboard", R.checkerboard(65, 130)
    for h, w in ((1, 1), (1, 300), (300, 1), (3, 5), (2, 64), (33, 3), (32, 64), (64, 128)):
        yield "noise3", R.noise(h, w, 3, seed=h + w)
        yield "checkerboard", R.checkerboard(h, w)
        yield "single", R.single(h, w, c=0)


# --------------------------------------------------------------------------- #
# 1. infur_regions_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conn", [4, 8])
def test_families_equal_the_reference(ctx, conn):
    assert ctx.L.infur_features() & _lib.FEATURE_REGIONS  # (the first line: fails on a library without the feature)
    counts = {}
    for name, k in small_families():
        counts[(name,) + k.shape] = check_against_reference(ctx, k, conn, name=name)[2]
    # what the families are for: the staircase and the checkerboard connect only diagonally, the paths are one region
    assert counts[("serpentine", 270, 480)] == 1 + (270 // 2) and counts[("spiral", 270, 480)] == 2
    assert counts[("checkerboard", 65, 130)] == (2 if conn == 8 else 65 * 130)
    assert counts[("single", 65, 130)] == 1 and counts[("noise3", 1, 1)] == 1
    if conn == 4:
        assert counts[("staircase", 65, 130)] > 65 * 130 // 5
    else:
        assert counts[("staircase", 65, 130)] < 65 + 130


@pytest.mark.parametrize("conn", [4, 8])
def test_1080p_planes_equal_the_reference(ctx, conn):
    check_against_reference(ctx, R.smooth(1080, 1920), conn, name="smooth")
    if conn == 8:
        assert check_against_reference(ctx, R.single(1080, 1920), conn, name="single")[2] == 1
    else:
        assert check_against_reference(ctx, R.serpentine(1080, 1920), conn, name="serpentine")[2] == 1 + 540


@pytest.mark.parametrize("conn", [4, 8])
def test_min_pixels_skip_background_and_truncation(ctx, conn):
    for name, k in (("smooth", R.smooth(270, 480)), ("noise3", R.noise(65, 130, 3)), ("noise21", R.noise(270, 480, 21))):
        full = R.label(k, None, conn)[2]
        for min_pixels, flags in ((1, 0), (2, 0), (9, 0), (0, R.SKIP_BACKGROUND), (5, R.SKIP_BACKGROUND), (k.size + 1, 0)):
            rn = check_against_reference(ctx, k, conn, min_pixels, flags, name=name)[2]
            assert rn == full if (min_pixels <= 1 and not flags) else rn < full
        # a table with room for fewer rows than there are regions: a prefix, the complete count, complete labels
        conf = R.conf_for(k)
        rl, rt, rn = R.label(k, conf, conn, 2, 0)
        rows = max(1, rn // 3)
        assert rows < rn
        labels, table, n = dev_regions(ctx, k, conf, conn, 2, 0, table_rows=rows)
        assert n == rn and (labels == rl).all() and (table == rt[:rows]).all()  # (dev_regions checked the bytes behind the rows)
        assert labels[labels != NONE].max() == rn - 1 >= rows
    # conf == NULL: the sums of confidence are 0, everything else as with one
    k = R.smooth(33, 47)
    _, rt, rn = R.label(k, None, conn)
    _, table, n = dev_regions(ctx, k, None, conn, table_rows=rn)
    assert n == rn and (table == rt).all() and (table[:, R.SUM_CONF] == 0).all()


def test_runs_are_repeatable_and_contexts_agree(ctx):
    k = R.noise(270, 480, 3, seed=9)
    conf = R.conf_for(k)
    rn = R.label(k, None, 8)[2]
    first = dev_regions(ctx, k, conf, 8, table_rows=rn)
    again = dev_regions(ctx, k, conf, 8, table_rows=rn)  # nothing accumulates across calls
    other = dev_regions(ctx, R.smooth(270, 480), conf, 4, table_rows=rn)  # another plane in between
    third = dev_regions(ctx, k, conf, 8, table_rows=rn)
    with Context(device=0) as c2:
        second_ctx = dev_regions(c2, k, conf, 8, table_rows=rn)
    for run in (again, third, second_ctx):
        assert run[2] == first[2] == rn
        assert run[0].tobytes() == first[0].tobytes() and run[1].tobytes() == first[1].tobytes()
    assert other[2] != rn


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    k = R.noise(6, 7, 3)
    d = Dev(ctx, klass=42, labels=42 * 4, table=80 * 4, n=4)
    try:
        d.put("klass", k)
        P = d.ptr
        call = lambda conn=8, flags=0, hh=6, ww=7, kl=P["klass"], lab=P["labels"], tab=P["table"], n=P["n"]: L.infur_regions_dev(  # noqa: E731
            h, kl, None, hh, ww, conn, 0, flags, lab, tab, 4, n)
        for conn in (0, 1, 6, 9):
            assert call(conn=conn) == _lib.E_INVALID_ARG
        assert call(flags=2) == _lib.E_INVALID_ARG
        assert call(lab=None, tab=None, n=None) == _lib.E_INVALID_ARG  # all outputs NULL
        assert call(kl=None) == _lib.E_INVALID_ARG
        assert call(hh=65536, ww=65536) == _lib.E_INVALID_ARG and call(hh=0xFFFFFFFF, ww=1) == _lib.E_INVALID_ARG  # h*w >= 2^32 - 1
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in ("labels", "table", "n"))
        # an empty image: n_regions = 0 and nothing else
        for hh, ww in ((0, 7), (6, 0), (0, 0)):
            d.poison("n")
            assert call(hh=hh, ww=ww) == _lib.OK
            ctx.synchronize()
            assert d.get("n").view(np.uint32)[0] == 0 and (d.get("labels") == POISON).all() and (d.get("table") == POISON).all()
        assert call(hh=0, n=None) == _lib.OK
        assert call() == _lib.OK
        ctx.synchronize()
        assert d.get("n").view(np.uint32)[0] == R.label(k, None, 8)[2]
    finally:
        d.free()
    # the host-pointer call: the same rules, n_regions a host word
    n = C.c_uint32(77)
    lab = np.full((6, 7), 9, np.uint32)
    assert L.infur_regions(h, k.ctypes.data, None, 6, 7, 5, 0, 0, lab.ctypes.data, None, 0, C.addressof(n)) == _lib.E_INVALID_ARG
    assert L.infur_regions(h, k.ctypes.data, None, 6, 7, 4, 0, 0, None, None, 0, None) == _lib.E_INVALID_ARG
    assert L.infur_regions(h, k.ctypes.data, None, 0, 7, 4, 0, 0, lab.ctypes.data, None, 0, C.addressof(n)) == _lib.OK
    assert n.value == 0 and (lab == 9).all()
    with pytest.raises(InfurError):
        Regions(ctx).control(RegionsCmd.Connectivity(5))


@pytest.mark.parametrize("conn", [4, 8])
def test_each_output_alone_equals_all_together(ctx, conn):
    for k in (R.smooth(270, 480), R.noise(65, 130, 3), R.noise(3, 5, 3)):
        conf = R.conf_for(k)
        rl, rt, rn = R.label(k, conf, conn, 2, R.SKIP_BACKGROUND)
        for want in (("labels",), ("table",), ("n",), ("labels", "n"), ("table", "n")):
            labels, table, n = dev_regions(ctx, k, conf, conn, 2, R.SKIP_BACKGROUND, table_rows=rn, want=want)
            assert labels is None or (labels == rl).all(), want
            assert table is None or (table == rt).all(), want
            assert n is None or n == rn, want
        # a table pointer with no rows is no table
        labels, table, n = dev_regions(ctx, k, conf, conn, 2, R.SKIP_BACKGROUND, table_rows=0)
        assert (labels == rl).all() and n == rn


@pytest.mark.parametrize("conn", [4, 8])
def test_host_pointer_call_and_processor(ctx, conn):
    reg = Regions(ctx, conn)
    for k in (R.smooth(270, 480), R.noise(65, 130, 21), R.serpentine(33, 200)):
        conf = R.conf_for(k)
        rl, rt, rn = R.label(k, conf, conn)
        out = RegionsOut(table_rows=rn + 5)
        reg.advance((k, conf), out)
        assert out.n == rn and (out.labels == rl).all() and out.table.shape == (rn, 10) and (out.table == rt).all()
        # the caller's rows beyond n, and beyond table_rows, are left alone
        labels = np.full(k.shape, 7, np.uint32)
        table = np.full((rn + 2, 10), 7, np.uint64)
        n = C.c_uint32(0)
        ctx.check(ctx.L.infur_regions(ctx.h, k.ctypes.data, conf.ctypes.data, k.shape[0], k.shape[1], conn, 0, 0, labels.ctypes.data,
                                      table.ctypes.data, rn + 2, C.addressof(n)))
        assert n.value == rn and (labels == rl).all() and (table[:rn] == rt).all() and (table[rn:] == 7).all()
        table[:] = 7
        ctx.check(ctx.L.infur_regions(ctx.h, k.ctypes.data, None, k.shape[0], k.shape[1], conn, 0, 0, None, table.ctypes.data, 1, C.addressof(n)))
        assert n.value == rn and (table[0, :3] == rt[0, :3]).all() and table[0, R.SUM_CONF] == 0 and (table[1:] == 7).all()
    reg.control(RegionsCmd.MinPixels(4)).control(RegionsCmd.Flags(_lib.REGIONS_SKIP_BACKGROUND))
    out = RegionsOut(want_labels=False, table_rows=2)
    reg.advance((k, None), out)
    rl, rt, rn = R.label(k, None, conn, 4, R.SKIP_BACKGROUND)
    assert out.labels is None and out.n == rn and (out.table == rt[:2]).all()


# --------------------------------------------------------------------------- #
# 2. the fused frame path
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_segments_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    for (h, w), factor, conn in (((61, 97), 1.0, 8), ((240, 320), 1.0, 4), ((240, 320), 0.5, 8), ((540, 960), 1.0, 8)):
        frame = W.synth_frame(h, w, index=h)
        s = fp.advance_segments(frame, factor, decode)
        rl, rt, rn = R.label(s.klass, s.conf, conn)
        r = fp.advance_regions(frame, factor, decode, conn, table_rows=rn + 1, want_scaled=True)
        assert r.klass.tobytes() == s.klass.tobytes() and r.conf.tobytes() == s.conf.tobytes(), (h, w, factor)
        assert r.n == rn and (r.labels == rl).all() and (r.table == rt).all(), (h, w, factor, conn)
        assert r.scaled.shape == s.klass.shape + (3,)
        lo, _ = model.lowres()  # infur_model_read_lowres still works afterwards
        assert lo.size > 0 and np.isfinite(lo).all()
        # filters, a truncated table, and the planes left in the library's scratch
        rl2, rt2, rn2 = R.label(s.klass, s.conf, conn, 6, R.SKIP_BACKGROUND)
        q = fp.advance_regions(frame, factor, decode, conn, 6, R.SKIP_BACKGROUND, table_rows=2, want_klass=False, want_conf=False)
        assert q.klass is None and q.conf is None and q.n == rn2 and (q.labels == rl2).all() and (q.table == rt2[:2]).all()
        recs = region_summary(r.table, r.n, s.klass.shape[1], s.klass.shape[0])
        assert sum(x["pixels"] for x in recs) == s.klass.size
        per_class = {c["klass"]: c["pixels"] for c in class_summary(s.stats, s.klass.shape[1], s.klass.shape[0])}
        assert {k: sum(x["pixels"] for x in recs if x["klass"] == k) for k in per_class} == per_class


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    for hh, ww in ((52, 100), (50, 99)):
        frame = W.synth_frame(hh, ww, index=2)
        hw = hh * ww
        s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
        rl, rt, rn = R.label(s.klass, s.conf, 8)
        d = Dev(ctx, bgr=frame.nbytes, klass=hw, conf=hw, labels=hw * 4, table=(rn + 2) * 80, n=4)
        try:
            d.put("bgr", frame)
            ow, oh = C.c_uint32(0), C.c_uint32(0)
            P = d.ptr
            for planes in (True, False):  # the caller's planes / the library's scratch
                d.poison("klass", "conf", "labels", "table", "n")
                ctx.check(L.infur_frame_regions_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 8, 0, 0, P["klass"] if planes else None,
                                                    P["conf"] if planes else None, hw, P["labels"], hw * 4, P["table"], rn + 2, P["n"], None,
                                                    C.byref(ow), C.byref(oh)))
                ctx.synchronize()
                assert (ow.value, oh.value) == (ww, hh)
                table = d.get("table").view(np.uint64).reshape(rn + 2, 10)
                assert d.get("n").view(np.uint32)[0] == rn and (d.get("labels").view(np.uint32) == rl.ravel()).all()
                assert (table[:rn] == rt).all() and (table[rn:].view(np.uint8) == POISON).all()
                if planes:
                    assert (d.get("klass") == s.klass.ravel()).all() and (d.get("conf") == s.conf.ravel()).all()
                else:
                    assert (d.get("klass") == POISON).all() and (d.get("conf") == POISON).all()
        finally:
            d.free()


def test_fused_rules_and_error_codes(ctx, model):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    kl, cf, lab = np.zeros((48, 64), np.uint8), np.zeros((48, 64), np.uint8), np.zeros((48, 64), np.uint32)
    tab = np.zeros((16, 10), np.uint64)
    n, ow, oh = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(decode=0, conn=8, flags=0, klass=kl, conf=cf, plane_cap=48 * 64, labels=lab, labels_cap=48 * 64 * 4, table=tab, count=n, mode=0,
             factor=1.0):
        return L.infur_frame_regions(h, p(frame), 64, 48, factor, mode, decode, conn, 0, flags, p(klass), p(conf), plane_cap, p(labels), labels_cap,
                                     p(table), 16, C.addressof(count) if count is not None else None, None, C.byref(ow), C.byref(oh))

    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48) and n.value == R.label(kl, None, 8)[2]
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) == _lib.E_INVALID_ARG
    assert call(conn=5) == _lib.E_INVALID_ARG and call(flags=4) == _lib.E_INVALID_ARG
    assert call(labels=None, table=None, count=None) == _lib.E_INVALID_ARG
    assert call(plane_cap=48 * 64 - 1) == _lib.E_CAPACITY
    assert call(klass=None, conf=None, plane_cap=0) == _lib.OK  # no plane wanted: its capacity does not matter
    assert call(labels_cap=48 * 64 * 4 - 1) == _lib.E_CAPACITY
    assert call(labels=None, labels_cap=0) == _lib.OK
    assert call(factor=-1.0) == _lib.E_INVALID_SCALE
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_regions(frame, 0.5, RAW, want_scaled=True)
        assert r.klass is None and r.labels is None and r.n is None and r.scaled.shape == (24, 32, 3)
        assert (r.scaled == FramePath(c).advance_segments(frame, 0.5, RAW, want_scaled=True).scaled).all()
        rc = c.L.infur_frame_regions(c.h, p(frame), 64, 48, 1.0, 0, 0, 8, 0, 0, None, None, 0, p(lab), 48 * 64 * 4, None, 0, None, None,
                                     C.byref(ow), C.byref(oh))
        assert rc == _lib.E_MODEL_NOT_LOADED


def test_regions_calls_leave_the_cached_graphs_alone(blob50):
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
            args = (fr, 1.0, SOFTMAX if it & 1 else RAW, 4 if it & 2 else 8)
            s = fg.advance_regions(*args, want_klass=bool(it & 4), want_conf=bool(it & 4))
            e = fe.advance_regions(*args)
            assert s.n == e.n and (s.labels == e.labels).all() and (s.table == e.table).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a regions call caused a capture"
        assert cached1 >= cached0, "a regions call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the regions calls were not replayed"


# --------------------------------------------------------------------------- #
# 3. the command line
# --------------------------------------------------------------------------- #
def test_cli_round_trip(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input", str(clip)]

    def cli(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return [json.loads(line) for line in r.stdout.splitlines()]

    plain = cli("--labels-out", str(tmp_path / "plain.u8"))
    assert len(plain) == 2 and all(sorted(rec) == ["classes", "frame", "height", "width"] for rec in plain)  # the format without the flag
    recs = cli("--regions", "--connectivity", "4", "--min-pixels", "3", "--skip-background", "--labels-out", str(tmp_path / "klass.u8"),
               "--regions-out", str(tmp_path / "labels.u32"), "--conf-out", str(tmp_path / "conf.u8"), "--max-regions", str(96 * 128))
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    conf = np.frombuffer((tmp_path / "conf.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    for i, rec in enumerate(recs):
        assert sorted(rec) == ["classes", "frame", "height", "n_regions", "regions", "width"] and rec["frame"] == plain[i]["frame"]
        assert rec["classes"] == json.loads(json.dumps(class_summary(S.stats(klass[i], conf[i], 21), 128, 96)))
        rl, rt, rn = R.label(klass[i], conf[i], 4, 3, R.SKIP_BACKGROUND)
        assert rec["n_regions"] == rn and (labels[i] == rl).all()
        want = json.loads(json.dumps(region_summary(rt, rn, 128, 96)))
        assert rec["regions"] == want and len(want) == rn
