"""Split on the GPU: the segment plane, rows and counts of ``infur_split*`` and of the fused ``infur_frame_split`` against
tests/split_ref.py.  Everything is an integer, exact and a function of the inputs alone, so every comparison is ``==`` on whole
arrays.  Every output buffer is poisoned and guard-padded first: what a call must leave alone still holds the poison afterwards."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import regions_ref as R  # noqa: E402
import split_ref as S  # noqa: E402
from test_gpu_compare import FRAME_H, FRAME_W, POISON, Dev  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd import weights as W  # noqa: E402
from infur_amd.processors import Context, FramePath, Model, ModelCmd, split_core  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
GUARD = 16  # words
CORES = (0, 4, 16, 64, NONE)
SHAPES = ((1, 1), (1, 70), (70, 1), (25, 52), (33, 63), (65, 130))
PLANES = {"dumbbell": S.dumbbell, "bar": S.bar, "band": S.band}
PLANES.update({f"smooth{h}x{w}": functools.partial(R.smooth, h, w, 5, 4, 8) for h, w in SHAPES})
PLANES["ties"] = functools.partial(R.smooth, 33, 63, 2, 3, 8)  # under heights that are no distance transform: ties, zeros, the largest
PLANES.update({f"one{h}x{w}": functools.partial(np.full, (h, w), 3, np.uint8) for h, w in SHAPES})


@functools.lru_cache(maxsize=None)
def plane_of(name, skip):
    """-> (plane u8, its dist2): computed once and left unchanged"""
    p = PLANES[name]()
    return p, S.dist2(p, skip) if name != "ties" else np.random.default_rng(11).choice(np.array([0, 1, 2, 3, 7, NONE], np.uint32), size=p.shape)


@functools.lru_cache(maxsize=None)
def reference(name, skip, core, slots=1 << 20):
    p, d = plane_of(name, skip)
    return S.split(p, d, core, skip, slots=slots)


def padded(words):
    a = np.full(words + 2 * GUARD, POISON * 0x01010101, np.uint32)
    return a, a[GUARD:GUARD + words]


def host_split(ctx, plane, height, core, skip=None, rows=None, slots=0, want=("labels", "table", "counts")):
    """infur_split on poisoned, guard-padded buffers -> {labels, table (as the buffer holds it), counts}, None where not wanted"""
    h, w = plane.shape
    rows = h * w if rows is None else rows
    full = {"labels": padded(h * w), "table": padded(rows * 6), "counts": padded(8)}
    p = lambda n: full[n][1].ctypes.data if n in want else None  # noqa: E731
    ctx.check(ctx.L.infur_split(ctx.h, plane.ctypes.data, plane.dtype.itemsize, height.ctypes.data, h, w, _lib.SPLIT_SKIP if skip is not None else 0,
                                skip or 0, core, slots, p("labels"), p("table"), rows, p("counts")))
    for name, (a, inner) in full.items():
        assert (a[:GUARD] == a[0]).all() and (a[-GUARD:] == a[0]).all() and a[0] == POISON * 0x01010101, f"the guard around {name} was written"
        if name not in want:
            assert (inner == a[0]).all(), f"{name} was not wanted and was written"
    return {"labels": full["labels"][1].reshape(h, w) if "labels" in want else None, "table": full["table"][1].reshape(rows, 6) if "table" in want else None,
            "counts": full["counts"][1] if "counts" in want else None}


def equal(got, ref, tag):
    labels, table, counts = ref
    if got["counts"] is not None:  # ROUNDS is the device's own: at most log2 of the unmarked basins and one, none when all are marked
        c, unmarked = got["counts"].copy(), int(counts[S.BASINS]) - int(counts[S.MARKED])
        assert c[S.ROUNDS] <= (unmarked.bit_length() + 1 if unmarked and not counts[S.STATUS] else 0), tag
        c[S.ROUNDS] = 0
        assert c.tolist() == counts.tolist(), tag
    if counts[S.STATUS] & S.OVERFLOW:  # nothing but the counts
        assert all(got[k] is None or (got[k].view(np.uint8) == POISON).all() for k in ("labels", "table")), tag
        return
    if got["labels"] is not None:
        assert (got["labels"] == labels).all(), tag
    if got["table"] is not None:
        n = min(len(table), len(got["table"]))
        assert (got["table"][:n] == table[:n]).all(), tag
        assert (got["table"][n:].view(np.uint8) == POISON).all(), tag  # what lies behind the rows is left alone


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("skip", (None, 0), ids=("keep", "skip0"))
@pytest.mark.parametrize("name", sorted(PLANES))
def test_planes_equal_the_reference(ctx, name, skip, core):
    if name.startswith("one") and skip == 0:
        skip = 3  # everything skipped
    plane, height = plane_of(name, skip)
    for dtype in (np.uint8, np.uint32):
        equal(host_split(ctx, plane.astype(dtype), height, core, skip), reference(name, skip, core), dtype)


def test_two_calls_give_identical_bytes(ctx):
    plane, height = plane_of("smooth65x130", None)
    first, _, again = (host_split(ctx, plane, height, core) for core in (4, 64, 4))  # another call's leavings lie in the scratch
    assert first["counts"][S.ROUNDS] > 0 and all(first[k].tobytes() == again[k].tobytes() for k in first)


@pytest.mark.parametrize("want", (("labels",), ("table",), ("counts",)))
def test_each_output_alone_truncated_rows_and_overflow(ctx, want):
    plane, height = plane_of("smooth33x63", None)
    ref = reference("smooth33x63", None, 4)
    assert ref[2][S.SEGMENTS] > 3 and 2 * ref[2][S.RUNS] > 64 and ref[2][S.SPLIT_VALUES] > 0
    equal(host_split(ctx, plane, height, 4, want=want), ref, want)
    equal(host_split(ctx, plane, height, 4, rows=3, want=want), ref, ("truncated",) + want)
    over = reference("smooth33x63", None, 4, slots=64)
    assert over[2][S.STATUS] == S.OVERFLOW
    equal(host_split(ctx, plane, height, 4, slots=64, want=want), over, ("overflow",) + want)


def test_the_device_chain_regions_anchors_split(ctx, model):
    """infur_frame_regions_dev -> infur_anchors_dev -> infur_split_dev on what each left in device memory"""
    L, hh, ww, core = ctx.L, FRAME_H, FRAME_W, 9
    frame = W.synth_frame(hh, ww, index=2)
    d = Dev(ctx, bgr=frame.nbytes, labels=hh * ww * 4, dist2=hh * ww * 4, seg=hh * ww * 4, table=256 * 24, counts=32)
    try:
        d.put("bgr", frame)
        P, ow, oh = d.ptr, C.c_uint32(0), C.c_uint32(0)
        ctx.check(L.infur_frame_regions_dev(ctx.h, P["bgr"], ww, hh, 1.0, 0, _lib.DECODE_SOFTMAX, 4, 0, 0, None, None, 0, P["labels"], hh * ww * 4, None, 0,
                                            None, None, C.byref(ow), C.byref(oh)))
        ctx.check(L.infur_anchors_dev(ctx.h, P["labels"], 4, hh, ww, 1, NONE, P["dist2"], None, 0))
        ctx.check(L.infur_split_dev(ctx.h, P["labels"], 4, P["dist2"], hh, ww, 1, NONE, core, 0, P["seg"], P["table"], 256, P["counts"]))
        ctx.synchronize()
        labels, dist2 = (d.get(k).view(np.uint32).reshape(hh, ww) for k in ("labels", "dist2"))
        ref = S.split(labels, dist2, core, NONE)
        got = {"labels": d.get("seg").view(np.uint32).reshape(hh, ww), "table": d.get("table").view(np.uint32).reshape(256, 6),
               "counts": d.get("counts").view(np.uint32)}
        assert ref[2][S.SEGMENTS] > 1
        equal(got, ref, "chain")
    finally:
        d.free()


def test_frame_split_beside_a_cached_graph(blob50):
    """infur_frame_split against the reference applied to infur_frame_anchors' own planes; the replayed leg keeps its graph"""
    frames = [W.synth_frame(120, 168, index=i) for i in range(2)]
    with Context(device=0, graph_replay=True) as cg:
        Model(cg).control(ModelCmd.LoadBlob(blob50))
        fp = FramePath(cg)
        for it in range(10):  # past the capture
            fp.advance(frames[it % 2], 1.0)
        cap0, rep0, cached0 = cg.graph_stats()
        assert cap0 == 1 and cached0 == 1
        for fr in frames:
            a = fp.advance_anchors(fr, 1.0, _lib.DECODE_SOFTMAX, 4)
            s = fp.advance_split(fr, 9, 1.0, _lib.DECODE_SOFTMAX, 4, want_labels=True, want_dist2=True, split_rows=1 << 20)
            assert s.n == a.n and (s.labels == a.labels).all() and (s.dist2 == a.dist2).all() and (s.anchors == a.anchors).all()
            labels, table, counts = S.split(a.labels, a.dist2, 9, NONE)
            counts[S.ROUNDS] = s.counts[S.ROUNDS]
            assert s.counts.tolist() == counts.tolist() and (s.segments == labels).all() and (s.segment_table == table).all()
            few = fp.advance_split(fr, 9, 1.0, _lib.DECODE_SOFTMAX, 4, split_rows=2, want_segments=False)  # the planes in scratch
            assert (few.segment_table == table[:2]).all() and few.segments is None and few.labels is None
            fp.advance(fr, 1.0)
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0 and cached1 >= cached0 and rep1 == rep0 + 2


def test_cli_round_trip(tmp_path):
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    clip = tmp_path / "clip.bgr24"
    clip.write_bytes(b"".join(f.tobytes() for f in frames))
    r = subprocess.run([sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input",
                        str(clip), "--regions", "--connectivity", "4", "--max-regions", "12288", "--split", "5", "--regions-out",
                        str(tmp_path / "labels.u32"), "--split-out", str(tmp_path / "seg.u32")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    labels = np.frombuffer((tmp_path / "labels.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    seg = np.frombuffer((tmp_path / "seg.u32").read_bytes(), np.uint32).reshape(2, 96, 128)
    assert split_core(5) == 9
    for i, rec in enumerate(json.loads(line) for line in r.stdout.splitlines()):
        ref_labels, table, counts = S.split(labels[i], S.dist2(labels[i], NONE), 9, NONE)
        assert (seg[i] == ref_labels).all() and rec["split"]["segments"] == counts[S.SEGMENTS] == len(rec["segments"])
        assert [(s["region"], s["pixels"], s["anchor"]) for s in rec["segments"]] == \
               [(int(t[S.VALUE]), int(t[S.PIXELS]), [int(t[S.PEAK]) % 128, int(t[S.PEAK]) // 128]) for t in table]
