"""Centrelines on the GPU: the records, vertices and counts of ``infur_centrelines*`` and of the fused ``infur_frame_centrelines``
against tests/centrelines_ref.py.  Everything is an integer, exact and a function of the inputs alone, so every comparison is ``==``
on whole arrays.  Every output buffer is poisoned and guard-padded first."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import centrelines_ref as CL  # noqa: E402
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
WORD = POISON * 0x01010101
SIZES = ((1, 1), (1, 70), (70, 1), (2, 2), (33, 63), (65, 130), (113, 49))
# thinned by Skeleton's reference: the kind plane goes in
THINNED = {f"single{h}x{w}": functools.partial(R.single, h, w) for h, w in SIZES}
THINNED.update({f"smooth{h}x{w}": functools.partial(R.smooth, h, w, 5, 4, 8) for h, w in SIZES})
THINNED.update({f"noise{h}x{w}": functools.partial(R.noise, h, w, 3) for h, w in SIZES})
THINNED["plus130x130"] = functools.partial(S.plus, 130, 130)        # one node of degree 4
THINNED["checkerboard9x11"] = functools.partial(R.checkerboard, 9, 11)  # every node of degree 4, every branch one link


def drawn(h, w, *pixels, value=1):
    p = np.zeros((h, w), np.uint8)
    for y, x in pixels:
        p[y, x] = value
    return p


def lines370():
    """rows of horizontal lines two apart: 185 branches of 370 vertices.  Both scans of centrelines.hip run over the pixels, 1024 to a
    block: 134 block sums, one pass of the block-sum scan (``wide1030`` below reaches the second)"""
    p = np.zeros((370, 370), np.uint8)
    p[0::2] = 1
    return p


def wide1030():
    """1030 x 1030 = 1036 scan blocks of pixels: the block-sum scans of the darts and of the branches take a second pass, with a line, a
    ring and isolated pixels inside the last twelve blocks, whose sums only that pass scans"""
    p = np.zeros((1030, 1030), np.uint8)
    p[0, :] = p[2, 5:9] = 1
    p[1020, 3:900] = p[1022, 7] = p[1022, 9] = 2
    p[1024:1029, 100:105] = 3
    p[1025:1028, 101:104] = 0
    return p


RING = drawn(6, 7, (1, 2), (1, 3), (1, 4), (2, 1), (2, 5), (3, 1), (3, 5), (4, 2), (4, 3), (4, 4))  # no node: a ring of ten pixels
DRAWN = {
    "ring": lambda: RING,
    # two self-loops at the junction (3, 3): each is walked both ways from the same pixel, the smaller dart id alone decides
    "eight": lambda: drawn(7, 7, (0, 2), (0, 3), (0, 4), (1, 1), (1, 5), (2, 2), (2, 4), (3, 3), (4, 2), (4, 4), (5, 1), (5, 5), (6, 2), (6, 3), (6, 4)),
    "diagonal": lambda: np.eye(9, 12, dtype=np.uint8),
    "isolated": lambda: drawn(5, 9, (0, 0), (0, 2), (2, 4), (4, 8), (4, 6)),
    "line1x70": lambda: np.ones((1, 70), np.uint8),
    "serpentine65x130": lambda: R.serpentine(65, 130),  # one chain of 4257 links over many workgroups: every round works
    "two_rings": lambda: np.hstack([RING, 2 * RING]),
    "lines370": lines370,
    "wide1030": wide1030,
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (plane u8, kind or None, heights with 0 and the largest among them): computed once and left unchanged"""
    p = (THINNED.get(name) or DRAWN[name])()
    kind = S.skeleton(p)[0] if name in THINNED else None
    return p, kind, np.random.default_rng(7).choice(np.array([0, 1, 5, 1000, NONE], np.uint32), size=p.shape)


@functools.lru_cache(maxsize=None)
def reference(name, with_height=True, skip=0, corners=False, max_links=0):
    p, kind, hgt = inputs(name)
    return CL.centrelines(p, kind, hgt if with_height else None, skip, corners, max_links)


def host_centrelines(ctx, plane, kind, height, skip=0, corners=False, max_links=0, rows=None, vertex_rows=None, want=("records", "vertices", "counts")):
    """infur_centrelines on poisoned, guard-padded buffers -> (records, vertices, counts) as the buffers hold them, None where not wanted"""
    h, w = plane.shape
    rows = min(4 * h * w + 1, 1 << 14) if rows is None else rows  # more than any plane here has
    vertex_rows = min(8 * h * w + 1, 1 << 17) if vertex_rows is None else vertex_rows
    full = {"records": padded(rows * 8), "vertices": padded(vertex_rows), "counts": padded(8)}
    p = lambda n: full[n][1].ctypes.data if n in want else None  # noqa: E731
    flags = (_lib.CENTRELINES_SKIP if skip is not None else 0) | (_lib.CENTRELINES_CORNERS if corners else 0)
    ctx.check(ctx.L.infur_centrelines(ctx.h, plane.ctypes.data, plane.dtype.itemsize, kind.ctypes.data if kind is not None else None,
                                      height.ctypes.data if height is not None else None, h, w, flags, skip or 0, max_links, p("records"), rows, p("vertices"),
                                      vertex_rows, p("counts")))
    for name, (a, inner) in full.items():
        assert (a[:GUARD] == WORD).all() and (a[-GUARD:] == WORD).all(), f"the guard around {name} was written"
        assert name in want or (inner == WORD).all(), f"{name} was not wanted and was written"
    return tuple(full[n][1] if n in want else None for n in ("records", "vertices", "counts"))


def equal(got, ref, tag, rows=None, vertex_rows=None):
    """what the buffers hold is the reference's prefix, and poison beyond it"""
    for g, r, n, what in zip(got, ref, (rows, vertex_rows, None), ("records", "vertices", "counts")):
        if g is not None:
            r = r.ravel() if n is None else r[:n].ravel()
            assert (g[:r.size] == r).all() and (g[r.size:] == WORD).all(), (tag, what, g[:r.size + 8], r)


@pytest.mark.parametrize("name", sorted(THINNED))
def test_thinned_planes_equal_the_reference(ctx, name):
    plane, kind, height = inputs(name)
    equal(host_centrelines(ctx, plane, kind, height, 0), reference(name), "u8, SKIP and height")
    equal(host_centrelines(ctx, plane.astype(np.uint32), kind, None, None), reference(name, False, None), "u32, neither")


@pytest.mark.parametrize("name", sorted(DRAWN))
def test_hand_drawn_planes_without_a_kind_plane(ctx, name):
    plane, kind, height = inputs(name)
    ref = reference(name)
    assert kind is None and ref[2][CL.BRANCHES] == {"ring": 1, "eight": 2, "diagonal": 1, "isolated": 5, "line1x70": 1, "serpentine65x130": 1, "two_rings": 2,
                                                    "lines370": 185, "wide1030": 6}[name]
    assert ref[2][CL.RINGS] == {"ring": 1, "two_rings": 2, "wide1030": 1}.get(name, 0)
    equal(host_centrelines(ctx, plane, None, height, 0), ref, name)


@pytest.mark.parametrize("name", ("ring", "serpentine65x130", "smooth65x130"))
def test_corners(ctx, name):
    ref = reference(name, corners=True)
    assert ref[2][CL.VERTICES] < reference(name)[2][CL.VERTICES]
    equal(host_centrelines(ctx, *inputs(name), 0, True), ref, name)


@pytest.mark.parametrize("want", (("records",), ("vertices",), ("counts",)))
def test_each_output_alone(ctx, want):
    equal(host_centrelines(ctx, *inputs("smooth65x130"), want=want), reference("smooth65x130"), want)


def test_fewer_rows_than_there_are(ctx):
    ref = reference("smooth65x130")
    nb, nv = int(ref[2][CL.BRANCHES]) - 1, int(ref[2][CL.VERTICES]) - 1
    equal(host_centrelines(ctx, *inputs("smooth65x130"), rows=nb), ref, "records", rows=nb)
    equal(host_centrelines(ctx, *inputs("smooth65x130"), vertex_rows=nv), ref, "vertices", vertex_rows=nv)


def test_capacity_at_the_links_and_one_below(ctx):
    links = int(reference("smooth65x130")[2][CL.LINKS])
    equal(host_centrelines(ctx, *inputs("smooth65x130"), max_links=links), reference("smooth65x130"), "just enough")
    over = reference("smooth65x130", max_links=links - 1)
    assert over[2][CL.STATUS] == CL.OVERFLOW and over[2][CL.LINKS] == links and not over[2][CL.BRANCHES] and not len(over[0]) and not len(over[1])
    equal(host_centrelines(ctx, *inputs("smooth65x130"), max_links=links - 1), over, "one too few")


def test_rejected_calls_leave_the_poison_and_an_empty_plane_writes_zero_counts(ctx):
    plane = R.noise(6, 7, 3)
    (_, rec), (_, vert), (_, counts) = padded(16), padded(16), padded(8)
    call = lambda elem=1, hh=6, ww=7, flags=0, skip=0, pl=plane.ctypes.data, r=rec.ctypes.data, rows=2, v=vert.ctypes.data, vrows=16, c=counts.ctypes.data: \
        ctx.L.infur_centrelines(ctx.h, pl, elem, None, None, hh, ww, flags, skip, 0, r, rows, v, vrows, c)  # noqa: E731
    for bad in (dict(elem=2), dict(flags=4), dict(flags=1, skip=256), dict(hh=65536), dict(pl=None), dict(r=None, v=None, c=None), dict(rows=0, vrows=0, c=None)):
        assert call(**bad) == _lib.E_INVALID_ARG, bad
    assert all((a == WORD).all() for a in (rec, vert, counts))
    assert call(hh=0, pl=None) == _lib.OK and not counts.any() and (rec == WORD).all() and (vert == WORD).all()


def test_the_device_chain_regions_anchors_skeleton_centrelines(ctx, model):
    """infur_frame_regions_dev -> infur_anchors_dev -> infur_skeleton_dev -> infur_centrelines_dev on what each left in device memory,
    then the last call captured in a graph and replayed twice: after the call outside the capture it is launches only"""
    L, hh, ww, rows, vrows = ctx.L, FRAME_H, FRAME_W, 1 << 14, 1 << 16
    frame = W.synth_frame(hh, ww, index=2)
    d = Dev(ctx, bgr=frame.nbytes, labels=hh * ww * 4, dist2=hh * ww * 4, kind=hh * ww, records=rows * 32, vertices=vrows * 4, counts=32)
    hip, graph, exe = _hip(), C.c_void_p(None), C.c_void_p(None)
    try:
        d.put("bgr", frame)
        P, ow, oh, stream = d.ptr, C.c_uint32(0), C.c_uint32(0), C.c_void_p(ctx.stream)
        ctx.check(L.infur_frame_regions_dev(ctx.h, P["bgr"], ww, hh, 1.0, 0, _lib.DECODE_SOFTMAX, 4, 0, 0, None, None, 0, P["labels"], hh * ww * 4, None, 0,
                                            None, None, C.byref(ow), C.byref(oh)))
        ctx.check(L.infur_anchors_dev(ctx.h, P["labels"], 4, hh, ww, 1, NONE, P["dist2"], None, 0))
        ctx.check(L.infur_skeleton_dev(ctx.h, P["labels"], 4, P["dist2"], hh, ww, 1, NONE, 0, P["kind"], None, 0, None))
        call = lambda: L.infur_centrelines_dev(ctx.h, P["labels"], 4, P["kind"], P["dist2"], hh, ww, 1, NONE, 0, P["records"], rows, P["vertices"], vrows,  # noqa: E731
                                               P["counts"])
        read = lambda: tuple(d.get(k).view(np.uint32) for k in ("records", "vertices", "counts"))  # noqa: E731
        ctx.check(call())
        ctx.synchronize()
        labels, dist2 = (d.get(k).view(np.uint32).reshape(hh, ww) for k in ("labels", "dist2"))
        ref = CL.centrelines(labels, d.get("kind").reshape(hh, ww), dist2, NONE)
        assert 10 < ref[2][CL.BRANCHES] < rows and ref[2][CL.VERTICES] < vrows and not ref[2][CL.STATUS]
        equal(read(), ref, "eager")
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for replay in range(2):
            d.poison("records", "vertices", "counts")
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            equal(read(), ref, ("replay", replay))
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


def test_frame_centrelines_is_the_chain_of_references(ctx, model):
    fp, fr = FramePath(ctx), W.synth_frame(120, 168, index=1)
    s = fp.advance_skeleton(fr, 1.0, _lib.DECODE_SOFTMAX, 4, want_labels=True, want_dist2=True, skeleton_rows=16)
    c = fp.advance_centrelines(fr, 1.0, _lib.DECODE_SOFTMAX, 4, want_labels=True, want_dist2=True, skeleton_rows=16)
    assert c.n == s.n and all((getattr(c, k) == getattr(s, k)).all() for k in ("labels", "dist2", "kind", "skeleton_table", "counts"))
    ref = CL.centrelines(s.labels, s.kind, s.dist2, NONE)
    assert all(g.shape == r.shape and (g == r).all() for g, r in zip((c.records, c.vertices, c.centreline_counts), ref))
    few = fp.advance_centrelines(fr, 1.0, _lib.DECODE_SOFTMAX, 4, corners=True, record_rows=3, want_kind=False, skeleton_rows=0)  # the planes in scratch
    ref = CL.centrelines(s.labels, s.kind, s.dist2, NONE, corners=True)
    assert (few.records == ref[0][:3]).all() and (few.vertices == ref[1]).all() and (few.centreline_counts == ref[2]).all() and few.kind is None


def test_a_small_call_after_a_larger_one_is_what_a_fresh_context_gives(ctx):
    host_centrelines(ctx, *inputs("serpentine65x130"))
    got = host_centrelines(ctx, *inputs("smooth33x63"))
    with Context(device=0) as fresh:
        first = host_centrelines(fresh, *inputs("smooth33x63"))
    assert all(g.tobytes() == f.tobytes() for g, f in zip(got, first))
    equal(got, reference("smooth33x63"), "after a larger call")
