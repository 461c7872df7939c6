"""Skeleton on the GPU: the kind plane, rows and counts of ``infur_skeleton*`` and of the fused ``infur_frame_skeleton`` against
tests/skeleton_ref.py.  Everything is an integer, exact and a function of the inputs alone, ROUNDS and UNFINISHED included, so every
comparison is ``==`` on whole arrays.  Every output buffer is poisoned and guard-padded first."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import regions_ref as R  # noqa: E402
import skeleton_ref as S  # noqa: E402
from test_gpu_anchors import _hip  # noqa: E402
from test_gpu_compare import FRAME_H, FRAME_W, POISON, Dev  # noqa: E402
from test_gpu_segments_split import GUARD, padded  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd import weights as W  # noqa: E402
from infur_amd.processors import Context, FramePath  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ROWS = 6
# (111, 47) .. (113, 49): one below, at and one above the core tile, kSkCoreH = 112 rows by kSkCoreW = 48 columns (skeleton.hip)
SIZES = ((1, 1), (1, 70), (70, 1), (2, 2), (33, 63), (65, 130), (130, 65), (111, 47), (112, 48), (113, 49))
K = 8  # kSkK, the sub-iterations of one thin launch
PLANES = {f"single{h}x{w}": functools.partial(R.single, h, w) for h, w in SIZES}
PLANES.update({f"smooth{h}x{w}": functools.partial(R.smooth, h, w, 5, 4, 8) for h, w in SIZES})
PLANES.update({f"{f.__name__}{h}x{w}": functools.partial(f, h, w) for f in (R.serpentine, R.staircase, R.checkerboard) for h, w in ((65, 130), (113, 49))})
PLANES.update({f"noise{h}x{w}": functools.partial(R.noise, h, w, 3) for h, w in ((65, 130), (113, 49))})
PLANES["square2x2"] = functools.partial(np.ones, (2, 2), np.uint8)
PLANES["plus130x130"] = functools.partial(S.plus, 130, 130)  # the arms cross the seams at x = 48, 96 and y = 112


@functools.lru_cache(maxsize=None)
def plane_of(name):
    """-> (plane u8, heights with 0 and the largest among them): computed once and left unchanged"""
    p = PLANES[name]()
    return p, np.random.default_rng(7).choice(np.array([0, 1, 5, 1000, NONE], np.uint32), size=p.shape)


@functools.lru_cache(maxsize=None)
def reference(name, with_height, skip, max_rounds=0, rows=ROWS):
    p, hgt = plane_of(name)
    return S.skeleton(p, hgt if with_height else None, skip, max_rounds, rows)


def host_skeleton(ctx, plane, height, skip=None, max_rounds=0, rows=ROWS, want=("kind", "table", "counts")):
    """infur_skeleton on poisoned, guard-padded buffers -> (kind, table, counts), None where not wanted"""
    h, w = plane.shape
    full = {"kind": padded((h * w + 3) // 4), "table": padded(rows * 8), "counts": padded(8)}
    p = lambda n: full[n][1].ctypes.data if n in want else None  # noqa: E731
    ctx.check(ctx.L.infur_skeleton(ctx.h, plane.ctypes.data, plane.dtype.itemsize, height.ctypes.data if height is not None else None, h, w,
                                   _lib.SKELETON_SKIP if skip is not None else 0, skip or 0, max_rounds, p("kind"), p("table"), rows, p("counts")))
    for name, (a, inner) in full.items():
        assert (a[:GUARD] == a[0]).all() and (a[-GUARD:] == a[0]).all() and a[0] == POISON * 0x01010101, f"the guard around {name} was written"
        if name not in want:
            assert (inner == a[0]).all(), f"{name} was not wanted and was written"
    kind = full["kind"][1].view(np.uint8)
    assert (kind[h * w:] == POISON).all()
    return (kind[:h * w].reshape(h, w) if "kind" in want else None, full["table"][1].reshape(rows, 8) if "table" in want else None,
            full["counts"][1] if "counts" in want else None)


def equal(got, ref, tag):
    for g, r, what in zip(got, ref, ("kind", "table", "counts")):
        assert g is None or (g.shape == r.shape and (g == r).all()), (tag, what, g, r)


@pytest.mark.parametrize("name", sorted(PLANES))
def test_planes_equal_the_reference(ctx, name):
    plane, height = plane_of(name)
    skip = int(plane.flat[0]) if name.startswith(("smooth", "plus")) else None
    equal(host_skeleton(ctx, plane, height, skip), reference(name, True, skip), "u8")
    equal(host_skeleton(ctx, plane.astype(np.uint32), None, None), reference(name, False, None), "u32, no height, nothing skipped")


@pytest.mark.parametrize("max_rounds", (0, 1, 2, K - 1, K, K + 1, 3 * K))
@pytest.mark.parametrize("name", ("single65x130", "smooth130x65", "plus130x130"))
def test_a_truncated_result_is_the_reference_at_the_same_max_rounds(ctx, name, max_rounds):
    plane, height = plane_of(name)
    ref = reference(name, True, None, max_rounds)
    assert name != "single65x130" or ref[2][S.ROUNDS] == (64 if max_rounds == 0 else max_rounds)  # the front crosses every seam
    equal(host_skeleton(ctx, plane, height, None, max_rounds), ref, max_rounds)


@pytest.mark.parametrize("want", (("kind",), ("table",), ("counts",)))
def test_each_output_alone_and_fewer_rows_than_values(ctx, want):
    plane, height = plane_of("smooth65x130")
    assert reference("smooth65x130", True, None)[1][:4, S.PIXELS].all() and plane.max() == 3  # four values keep pixels: two rows are fewer
    equal(host_skeleton(ctx, plane, height, want=want), reference("smooth65x130", True, None), want)
    equal(host_skeleton(ctx, plane, height, rows=2, want=want), reference("smooth65x130", True, None, rows=2), ("two rows",) + want)


def test_rejected_calls_leave_the_poison_and_an_empty_plane_writes_empty_rows(ctx):
    plane = R.noise(6, 7, 3)
    (_, kind), (_, table), (_, counts) = padded(11), padded(16), padded(8)
    call = lambda elem=1, hh=6, ww=7, flags=0, skip=0, rounds=0, pl=plane.ctypes.data, k=kind.ctypes.data, t=table.ctypes.data, rows=2, c=counts.ctypes.data: \
        ctx.L.infur_skeleton(ctx.h, pl, elem, None, hh, ww, flags, skip, rounds, k, t, rows, c)  # noqa: E731
    for bad in (dict(elem=2), dict(flags=2), dict(skip=256), dict(hh=65536), dict(rounds=_lib.SKELETON_MAX_ROUNDS + 1), dict(pl=None),
                dict(k=None, t=None, c=None), dict(k=None, rows=0, c=None)):
        assert call(**bad) == _lib.E_INVALID_ARG, bad
    assert all((a.view(np.uint8) == POISON).all() for a in (kind, table, counts))
    assert call(hh=0, pl=None) == _lib.OK and table.tolist() == [0, 0, 0, 0, 0, NONE, 0, 0] * 2 and not counts.any() and (kind.view(np.uint8) == POISON).all()


def test_the_device_chain_regions_anchors_skeleton(ctx, model):
    """infur_frame_regions_dev -> infur_anchors_dev -> infur_skeleton_dev on what each left in device memory, then the same call
    captured in a graph and replayed twice: after the call outside the capture it is launches only"""
    L, hh, ww, rows = ctx.L, FRAME_H, FRAME_W, 256
    frame = W.synth_frame(hh, ww, index=2)
    d = Dev(ctx, bgr=frame.nbytes, labels=hh * ww * 4, dist2=hh * ww * 4, kind=hh * ww, table=rows * 32, counts=32)
    hip, graph, exe = _hip(), C.c_void_p(None), C.c_void_p(None)
    try:
        d.put("bgr", frame)
        P, ow, oh, stream = d.ptr, C.c_uint32(0), C.c_uint32(0), C.c_void_p(ctx.stream)
        ctx.check(L.infur_frame_regions_dev(ctx.h, P["bgr"], ww, hh, 1.0, 0, _lib.DECODE_SOFTMAX, 4, 0, 0, None, None, 0, P["labels"], hh * ww * 4, None, 0,
                                            None, None, C.byref(ow), C.byref(oh)))
        ctx.check(L.infur_anchors_dev(ctx.h, P["labels"], 4, hh, ww, 1, NONE, P["dist2"], None, 0))
        call = lambda: L.infur_skeleton_dev(ctx.h, P["labels"], 4, P["dist2"], hh, ww, 1, NONE, 0, P["kind"], P["table"], rows, P["counts"])  # noqa: E731
        read = lambda: (d.get("kind").reshape(hh, ww), d.get("table").view(np.uint32).reshape(rows, 8), d.get("counts").view(np.uint32))  # noqa: E731
        ctx.check(call())
        ctx.synchronize()
        labels, dist2 = (d.get(k).view(np.uint32).reshape(hh, ww) for k in ("labels", "dist2"))
        ref = S.skeleton(labels, dist2, NONE, 0, rows)
        assert ref[2][S.KEPT] > 10 and ref[2][S.ROUNDS] > K and not ref[2][S.STATUS]
        equal(read(), ref, "eager")
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for replay in range(2):
            d.poison("kind", "table", "counts")
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            equal(read(), ref, ("replay", replay))
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


def test_frame_skeleton_is_the_chain_of_references(ctx, model):
    fp, fr = FramePath(ctx), W.synth_frame(120, 168, index=1)
    a = fp.advance_anchors(fr, 1.0, _lib.DECODE_SOFTMAX, 4)
    s = fp.advance_skeleton(fr, 1.0, _lib.DECODE_SOFTMAX, 4, want_labels=True, want_dist2=True, skeleton_rows=1 << 20)
    assert s.n == a.n and (s.labels == a.labels).all() and (s.dist2 == a.dist2).all() and (s.anchors == a.anchors).all()
    ref = S.skeleton(a.labels, a.dist2, NONE, 0, a.labels.size)
    equal((s.kind, s.skeleton_table, s.counts), ref, "frame")
    few = fp.advance_skeleton(fr, 1.0, _lib.DECODE_SOFTMAX, 4, skeleton_rows=2, max_rounds=3, want_kind=False)  # the planes in scratch
    equal((None, few.skeleton_table, few.counts), S.skeleton(a.labels, a.dist2, NONE, 3, 2), "two rows, three sub-iterations")


def test_a_small_call_after_a_larger_one_is_what_a_fresh_context_gives(ctx):
    big, small = plane_of("single130x65"), plane_of("smooth33x63")
    host_skeleton(ctx, *big)
    got = host_skeleton(ctx, *small)
    with Context(device=0) as fresh:
        first = host_skeleton(fresh, *small)
    assert all(g.tobytes() == f.tobytes() for g, f in zip(got, first))
    equal(got, reference("smooth33x63", True, None), "after a larger call")
