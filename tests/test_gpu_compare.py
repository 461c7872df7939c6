"""Compare on the GPU: the matrix, the two row tables and the counts of ``infur_compare*`` and of the fused ``infur_frame_compare*``
against tests/compare_ref.py.  Everything is an integer, exact and a function of the two planes alone, so every comparison is
``==`` on whole arrays.  Every output buffer is filled with a poison byte first: what a call must leave alone still holds it
afterwards, and what it must write owes nothing to an initialisation."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd import weights as W
from infur_amd.processors import Compare, CompareCmd, CompareOut, Context, FramePath, Model, ModelCmd, confusion_summary, panoptic_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_ref as CR  # noqa: E402
import regions_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RAW, SOFTMAX = _lib.DECODE_RAW, _lib.DECODE_SOFTMAX
IGN_A, IGN_B = _lib.COMPARE_IGNORE_A, _lib.COMPARE_IGNORE_B
NONE = 0xFFFFFFFF
GUARD = 64
POISON = 0xA5
OUTPUTS = ("matrix", "a", "b", "counts")


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


def out_sizes(rows_a, rows_b):
    return dict(matrix=rows_a * rows_b * 4, a=rows_a * 16, b=rows_b * 16, counts=32)


def read_outputs(d, rows_a, rows_b, want):
    """the four outputs of a call as arrays, None for what was not wanted (and that buffer is checked to be untouched)"""
    got = {"matrix": d.get("matrix").view(np.uint32).reshape(rows_a, rows_b), "a": d.get("a").view(np.uint32).reshape(rows_a, 4),
           "b": d.get("b").view(np.uint32).reshape(rows_b, 4), "counts": d.get("counts").view(np.uint32)}
    for name in OUTPUTS:
        if name not in want:
            assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not wanted and was written"
            got[name] = None
    return got


def dev_compare(ctx, a, b, flags=0, ignore_a=0, ignore_b=0, rows_a=0, rows_b=0, pair_slots=0, want=OUTPUTS):
    """infur_compare_dev on poisoned device buffers -> {matrix, a, b, counts}"""
    h, w = a.shape
    d = Dev(ctx, pa=a.nbytes, pb=b.nbytes, **out_sizes(rows_a, rows_b))
    try:
        d.put("pa", a)
        d.put("pb", b)
        p = lambda name: d.ptr[name] if name in want else None  # noqa: E731
        ctx.check(ctx.L.infur_compare_dev(ctx.h, d.ptr["pa"], a.dtype.itemsize, d.ptr["pb"], b.dtype.itemsize, h, w, flags, ignore_a, ignore_b, p("matrix"),
                                          rows_a, rows_b, p("a"), p("b"), p("counts"), pair_slots))
        ctx.synchronize()
        assert d.get("pa").tobytes() == a.tobytes() and d.get("pb").tobytes() == b.tobytes()  # the inputs are inputs
        return read_outputs(d, rows_a, rows_b, want)
    finally:
        d.free()


_PLANES = {}


@functools.lru_cache(maxsize=None)
def _reference(ka, kb, flags, ignore_a, ignore_b, rows_a, rows_b, pair_slots):
    return CR.compare(_PLANES[ka], _PLANES[kb], flags, ignore_a, ignore_b, rows_a, rows_b, pair_slots)


def reference(a, b, flags=0, ignore_a=0, ignore_b=0, rows_a=0, rows_b=0, pair_slots=0):
    """the reference's answer, computed once per pair of planes and setting, and left unchanged"""
    keys = []
    for p in (a, b):
        key = (p.shape, p.dtype.str, p.tobytes())
        _PLANES.setdefault(key, p)
        keys.append(key)
    return _reference(keys[0], keys[1], flags, ignore_a, ignore_b, rows_a, rows_b, pair_slots)


def equal(got, ref, table_bit=None):
    """every wanted output == the reference's; table_bit: the form the case must have exercised"""
    for name in OUTPUTS:
        if got[name] is not None:
            assert (got[name] == getattr(ref, name)).all(), name
    if table_bit is not None and got["counts"] is not None:
        assert bool(got["counts"][CR.STATUS] & CR.TABLE) == table_bit
    return True


def check(ctx, a, b, name="", **kw):
    ref = reference(a, b, **kw)
    got = dev_compare(ctx, a, b, **kw)
    print(f"{name} {a.shape[0]}x{a.shape[1]} {a.dtype}/{b.dtype} {kw}: counts {ref.counts.tolist()}")
    for out in OUTPUTS:
        assert (got[out] == getattr(ref, out)).all(), (name, a.shape, a.dtype, b.dtype, kw, out)
    return ref


def labels_of(k):
    """(label plane u32, number of regions) of a class plane, small regions dropped: the plane holds NONE"""
    labels, _, n = R.label(k, None, 8, min_pixels=3, flags=0)
    return labels, n


def plane_pairs(h, w):
    sm = R.smooth(h, w, seed=h + w)
    yield "smooth/shifted", sm, CR.shifted(sm, min(1, h - 1), min(2, w - 1)), 21
    yield "noise2/noise3", R.noise(h, w, 2, seed=w), R.noise(h, w, 3, seed=h), 3
    yield "identical", R.noise(h, w, 21, seed=5), R.noise(h, w, 21, seed=5), 21
    yield "single/noise", R.single(h, w), R.noise(h, w, 21, seed=h + 1), 21


SHAPES = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (135, 241), (300, 3), (2, 16500))
ELEMS = ((np.uint8, np.uint8), (np.uint8, np.uint32), (np.uint32, np.uint8), (np.uint32, np.uint32))


# --------------------------------------------------------------------------- #
# 1. infur_compare_dev against the reference
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("ea,eb", ELEMS)
def test_plane_pairs_equal_the_reference(ctx, ea, eb):
    assert ctx.L.infur_features() & _lib.FEATURE_COMPARE  # (the first line: fails on a library without the feature)
    for h, w in SHAPES:
        for name, a, b, k in plane_pairs(h, w):
            a, b = a.astype(ea), b.astype(eb)
            ref = check(ctx, a, b, name, rows_a=k, rows_b=k)  # dense
            assert ref.counts[CR.STATUS] == 0 and ref.counts[CR.OUTSIDE] == 0 and ref.counts[CR.COMPARED] == h * w
            ref = check(ctx, a, b, name, rows_a=64, rows_b=65)  # the same data through the table
            assert ref.counts[CR.STATUS] == CR.TABLE
            ign = int(b[-1, -1])
            check(ctx, a, b, name, flags=IGN_B, ignore_b=ign, rows_a=k, rows_b=k)
            check(ctx, a, b, name, flags=IGN_A | IGN_B, ignore_a=int(a[0, 0]), ignore_b=ign, rows_a=70, rows_b=60)


def test_label_planes_of_regions(ctx):
    for h, w in ((33, 63), (135, 241)):
        ka = R.smooth(h, w, seed=h, cell=12)
        (la, na), (lb, nb) = labels_of(ka), labels_of(CR.shifted(ka, 2, 3))
        assert (la == NONE).any() and (na * nb > 4096) == (h == 135)  # the small plane is the dense form, the large one the table
        ref = check(ctx, la, lb, "labels", flags=IGN_A | IGN_B, ignore_a=NONE, ignore_b=NONE, rows_a=na, rows_b=nb)
        assert ref.counts[CR.IGNORED] > 0 and ref.counts[CR.OUTSIDE] == 0 and ref.counts[CR.MATCHED] > 0
        ref = check(ctx, la, lb, "labels, NONE outside", rows_a=na, rows_b=nb)  # not ignored: 0xFFFFFFFF is a value above rows
        assert ref.counts[CR.OUTSIDE] > 0 == ref.counts[CR.IGNORED]
        check(ctx, la, ka, "labels against classes", flags=IGN_A, ignore_a=NONE, rows_a=na, rows_b=21)
    # a label plane against itself: every region is matched with IoU 1, and the summaries say PQ = 1
    got = dev_compare(ctx, la, la, IGN_A, NONE, 0, na, na)
    assert got["counts"][CR.MATCHED] == na == got["counts"][CR.PAIRS] and (got["a"][:, CR.INTER] == got["a"][:, CR.UNION]).all()
    klass = [int(ka.ravel()[np.flatnonzero(la.ravel() == i)[0]]) for i in range(na)]
    assert panoptic_summary(got["a"], got["b"], klass, klass)["pq"] == 1.0


@pytest.mark.parametrize("shape", [(1, 65535), (65535, 1)])
def test_the_longest_sides(ctx, shape):
    h, w = shape
    a, b = R.noise(h, w, 3, seed=1), R.noise(h, w, 3, seed=2)
    ref = check(ctx, a, b, "noise3", rows_a=3, rows_b=3)
    assert ref.counts[CR.RUNS] > 30000 and ref.counts[CR.PAIRS] == 9
    check(ctx, a, b.astype(np.uint32), "noise3", rows_a=64, rows_b=65)


def test_both_forms_at_the_edge_of_the_rule(ctx):
    """64 x 64 values is the dense form, 64 x 65 and 65 x 64 the table: on the same data every output is the same apart from
    the TABLE bit"""
    a, b = R.noise(135, 241, 64, seed=3), R.noise(135, 241, 64, seed=4)
    dense = dev_compare(ctx, a, b, rows_a=64, rows_b=64)
    assert dense["counts"][CR.STATUS] == 0 and equal(dense, reference(a, b, rows_a=64, rows_b=64), table_bit=False)
    assert dense["counts"][CR.PAIRS] > 4000  # (nearly) every entry of the LDS matrix is in use
    for rows_a, rows_b in ((64, 65), (65, 64)):
        table = dev_compare(ctx, a, b, rows_a=rows_a, rows_b=rows_b)
        assert equal(table, reference(a, b, rows_a=rows_a, rows_b=rows_b), table_bit=True)
        assert table["counts"][CR.STATUS] == CR.TABLE and (table["counts"][:7] == dense["counts"][:7]).all()
        assert (table["matrix"][:64, :64] == dense["matrix"]).all() and table["matrix"].sum() == dense["matrix"].sum()
        assert (table["a"][:64] == dense["a"]).all() and (table["b"][:64] == dense["b"]).all()
    # the dense form's own edges: one row of 4096 values, and no values at all on one side
    wide = R.noise(33, 63, 200, seed=6)
    assert equal(dev_compare(ctx, R.single(33, 63, 0), wide, rows_a=1, rows_b=4096), reference(R.single(33, 63, 0), wide, rows_a=1, rows_b=4096), False)
    assert equal(dev_compare(ctx, wide, R.single(33, 63, 0), rows_a=4096, rows_b=1), reference(wide, R.single(33, 63, 0), rows_a=4096, rows_b=1), False)
    none = dev_compare(ctx, a, b, rows_a=0, rows_b=7)
    assert equal(none, reference(a, b, rows_a=0, rows_b=7), False) and none["counts"][CR.OUTSIDE] == a.size and (none["b"] == [0, NONE, 0, 0]).all()


def test_rows_below_equal_and_above_the_number_of_values(ctx):
    a, b = R.smooth(135, 241), R.smooth(135, 241, seed=7)
    top = max(int(a.max()), int(b.max())) + 1
    for rows_a, rows_b in ((1, 1), (top - 1, top), (top, top - 2), (top, top), (top + 9, top + 3), (top + 60, top + 60)):
        ref = check(ctx, a, b, "rows", rows_a=rows_a, rows_b=rows_b)
        assert (ref.counts[CR.OUTSIDE] > 0) == (rows_a < top or rows_b < top)
        assert (ref.a[top:] == [0, NONE, 0, 0]).all() and (ref.b[top:] == [0, NONE, 0, 0]).all()  # every row is written


@pytest.mark.parametrize("rows", [(21, 21), (80, 80)])
def test_ignore_off_on_each_side_and_on_both(ctx, rows):
    a, b = R.smooth(135, 241, seed=2), CR.shifted(R.smooth(135, 241, seed=2), 3, 5)
    ia, ib = int(a[60, 100]), int(b[10, 10])
    seen = set()
    for flags in (0, IGN_A, IGN_B, IGN_A | IGN_B):
        ref = check(ctx, a, b, "ignore", flags=flags, ignore_a=ia, ignore_b=ib, rows_a=rows[0], rows_b=rows[1])
        seen.add(int(ref.counts[CR.IGNORED]))
        assert int(ref.counts[CR.COMPARED]) + int(ref.counts[CR.IGNORED]) == a.size
    assert len(seen) == 4 and 0 in seen
    # a value that is ignored without its flag is compared
    assert check(ctx, a, b, "ignore", flags=IGN_A, ignore_a=ia, ignore_b=ib, rows_a=rows[0], rows_b=rows[1]).counts[CR.IGNORED] == (a == ia).sum()


@pytest.mark.parametrize("rows", [(3, 3), (64, 65)])
def test_each_output_alone_with_the_others_still_poison(ctx, rows):
    a, b = R.noise(33, 63, 3, seed=8), R.noise(33, 63, 3, seed=9).astype(np.uint32)
    ref = reference(a, b, rows_a=rows[0], rows_b=rows[1])
    for want in (("matrix",), ("a",), ("b",), ("counts",), ("a", "b"), ("matrix", "counts")):
        assert equal(dev_compare(ctx, a, b, rows_a=rows[0], rows_b=rows[1], want=want), ref), want


def test_overflow_is_visible_and_everything_else_exact(ctx):
    a, b = R.noise(135, 241, 3, seed=1), R.noise(135, 241, 3, seed=2)
    full = reference(a, b, rows_a=64, rows_b=65)
    got = dev_compare(ctx, a, b, rows_a=64, rows_b=65, pair_slots=64)
    ref = reference(a, b, rows_a=64, rows_b=65, pair_slots=64)
    assert equal(got, ref) and got["counts"][CR.STATUS] == CR.TABLE | CR.OVERFLOW
    assert (got["matrix"] == full.matrix).all() and (got["a"][:, CR.PIXELS] == full.a[:, CR.PIXELS]).all() and (got["counts"][:4] == full.counts[:4]).all()
    assert (got["a"][:, 1:] == [NONE, 0, 0]).all() and (got["b"][:, 1:] == [NONE, 0, 0]).all() and got["counts"][CR.PAIRS] == 0 == got["counts"][CR.MATCHED]
    assert got["counts"][CR.RUNS] == full.counts[CR.RUNS]
    # the dense form has no table: the same slots, the same noise, no overflow
    assert dev_compare(ctx, a, b, rows_a=3, rows_b=3, pair_slots=64)["counts"][CR.STATUS] == 0
    # 2 R == pair_slots exactly: no overflow; one run more: overflow
    exact = np.zeros((1, 70), np.uint8)
    exact[0, :31] = np.arange(31) % 2
    exact[0, 31:] = 2  # 31 runs, one up to column 63, one behind the cut at 64: 33
    exact = exact[:, :64]  # ... and 32 without it
    ref = check(ctx, exact, exact, "2R == slots", rows_a=64, rows_b=65, pair_slots=64)
    assert ref.counts[CR.RUNS] == 32 and ref.counts[CR.STATUS] == CR.TABLE and ref.counts[CR.PAIRS] == 3
    more = np.concatenate([exact, np.full((1, 1), 2, np.uint8)], axis=1)
    ref = check(ctx, more, more, "2R == slots + 2", rows_a=64, rows_b=65, pair_slots=64)
    assert ref.counts[CR.RUNS] == 33 and ref.counts[CR.STATUS] == CR.TABLE | CR.OVERFLOW


def test_calls_are_repeatable_and_contexts_agree(ctx):
    a, b = R.noise(135, 241, 3, seed=9), R.noise(135, 241, 3, seed=10)  # three values: thousands of atomics per address
    for rows in ((3, 3), (64, 65)):
        kw = dict(rows_a=rows[0], rows_b=rows[1])
        runs = [dev_compare(ctx, a, b, **kw) for _ in range(5)]
        big_a, big_b = R.smooth(270, 480), R.smooth(270, 480, seed=1)
        other = dev_compare(ctx, big_a, big_b, rows_a=rows[0] + 40, rows_b=rows[1] + 40)  # a larger plane and more rows in between: the scratch grows
        runs.append(dev_compare(ctx, a, b, **kw))
        with Context(device=0) as c2:
            runs.append(dev_compare(c2, a, b, **kw))
        for run in runs[1:]:
            assert all(run[name].tobytes() == runs[0][name].tobytes() for name in OUTPUTS)
        assert equal(runs[0], reference(a, b, **kw)) and equal(other, reference(big_a, big_b, rows_a=rows[0] + 40, rows_b=rows[1] + 40))
    # two calls in a row on one stream, no synchronisation between them: the second does not disturb the first's outputs
    d1, d2 = Dev(ctx, pa=a.nbytes, pb=b.nbytes, **out_sizes(3, 3)), Dev(ctx, **out_sizes(64, 65))
    try:
        d1.put("pa", a)
        d1.put("pb", b)
        for d, (ra, rb) in ((d1, (3, 3)), (d2, (64, 65))):
            ctx.check(ctx.L.infur_compare_dev(ctx.h, d1.ptr["pa"], 1, d1.ptr["pb"], 1, 135, 241, 0, 0, 0, d.ptr["matrix"], ra, rb, d.ptr["a"], d.ptr["b"],
                                              d.ptr["counts"], 0))
        ctx.synchronize()
        assert equal(read_outputs(d1, 3, 3, OUTPUTS), reference(a, b, rows_a=3, rows_b=3), False)
        assert equal(read_outputs(d2, 64, 65, OUTPUTS), reference(a, b, rows_a=64, rows_b=65), True)
    finally:
        d1.free()
        d2.free()


def _hip():
    """the HIP runtime this process already runs on (the one mapped file, not a second copy)"""
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [C.c_void_p]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize("rows", [(3, 3), (64, 65)])
def test_the_device_call_inside_a_captured_graph(ctx, rows):
    """after one call outside the capture the scratch is there: the call is memsets and launches, and a graph of them replays to
    the same bytes on whatever planes lie in the input buffers"""
    hip = _hip()
    h, w = 33, 63
    ra, rb = rows
    first = (R.noise(h, w, 3, seed=3), R.noise(h, w, 3, seed=4))
    second = (R.smooth(h, w, seed=5, classes=3), R.noise(h, w, 2, seed=6))
    d = Dev(ctx, pa=h * w, pb=h * w, **out_sizes(ra, rb))
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    try:
        P, stream = d.ptr, C.c_void_p(ctx.stream)
        call = lambda: ctx.L.infur_compare_dev(ctx.h, P["pa"], 1, P["pb"], 1, h, w, IGN_B, 0, 1, P["matrix"], ra, rb, P["a"], P["b"], P["counts"], 0)  # noqa: E731
        d.put("pa", first[0])
        d.put("pb", first[1])
        ctx.check(call())  # the warm call
        ctx.synchronize()
        assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
        rc = call()
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == _lib.OK and graph.value
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        for a, b in (second, first):
            d.poison(*OUTPUTS)
            d.put("pa", a)
            d.put("pb", b)
            assert hip.hipGraphLaunch(exe, stream) == 0
            ctx.synchronize()
            assert equal(read_outputs(d, ra, rb, OUTPUTS), reference(a, b, flags=IGN_B, ignore_b=1, rows_a=ra, rows_b=rb), ra * rb > 4096)
    finally:
        if exe.value:
            hip.hipGraphExecDestroy(exe)
        if graph.value:
            hip.hipGraphDestroy(graph)
        d.free()


def test_rules_and_error_codes(ctx):
    L, h = ctx.L, ctx.h
    a, b = R.noise(6, 7, 3, seed=1), R.noise(6, 7, 3, seed=2)
    d = Dev(ctx, pa=42 * 4, pb=42 * 4, **out_sizes(5, 5))
    try:
        d.put("pa", a.astype(np.uint32))
        d.put("pb", b.astype(np.uint32))
        P = d.ptr

        def call(ea=4, eb=4, flags=0, ia=0, ib=0, hh=6, ww=7, pa=P["pa"], pb=P["pb"], matrix=P["matrix"], ra=5, rb=5, oa=P["a"], ob=P["b"],
                 counts=P["counts"], slots=0):
            return L.infur_compare_dev(h, pa, ea, pb, eb, hh, ww, flags, ia, ib, matrix, ra, rb, oa, ob, counts, slots)

        bad = _lib.E_INVALID_ARG
        nothing = dict(matrix=None, oa=None, ob=None, counts=None)
        for e in (0, 2, 3, 8):
            assert call(ea=e) == bad and "elem_a" in ctx.last_error()
            assert call(eb=e) == bad and "elem_b" in ctx.last_error()
        assert call(flags=4) == bad and call(flags=7) == bad and "unknown compare flags" in ctx.last_error()
        assert call(ea=1, ia=256) == bad and "ignore_a" in ctx.last_error() and call(eb=1, flags=IGN_B, ib=256) == bad and "ignore_b" in ctx.last_error()
        assert call(hh=65536) == bad and call(ww=65536) == bad and "up to 65535" in ctx.last_error()
        for slots in (1, 32, 63, 65, 96, (1 << 20) + 1):
            assert call(slots=slots) == bad and "pair_slots" in ctx.last_error()  # in either form: these rows are the dense one
        assert call(**nothing) == bad and "no output wanted" in ctx.last_error()
        assert call(matrix=None, counts=None, ra=0, rb=0) == bad and "no output wanted" in ctx.last_error()  # tables without rows: not wanted
        assert call(ra=1024, rb=1025) == bad and "2^20" in ctx.last_error()
        assert call(pa=None) == bad and "no plane pointer" in ctx.last_error() and call(pb=None) == bad and "no plane pointer" in ctx.last_error()
        # the order of the checks, as the header states it
        worst = dict(ea=2, eb=2, flags=4, ia=256, ib=256, hh=65536, slots=3, pa=None, ra=1024, rb=1025)
        assert call(**worst) == bad and "elem_a" in ctx.last_error()
        worst["ea"] = 1
        assert call(**worst) == bad and "elem_b" in ctx.last_error()
        worst["eb"] = 1
        assert call(**worst) == bad and "flags" in ctx.last_error()
        worst["flags"] = 0
        assert call(**worst) == bad and "ignore_a" in ctx.last_error()
        worst["ia"] = 0
        assert call(**worst) == bad and "ignore_b" in ctx.last_error()
        worst["ib"] = 0
        assert call(**worst) == bad and "up to 65535" in ctx.last_error()
        worst["hh"] = 6
        assert call(**worst) == bad and "pair_slots" in ctx.last_error()
        worst["slots"] = 64
        assert call(**worst, **nothing) == bad and "no output wanted" in ctx.last_error()
        assert call(**worst) == bad and "2^20" in ctx.last_error()
        worst["ra"] = 5
        assert call(**worst) == bad and "no plane pointer" in ctx.last_error()
        ctx.synchronize()
        assert all((d.get(name) == POISON).all() for name in OUTPUTS)  # no output is touched by a rejected call
        # row tables above 2^20 entries without a matrix are fine
        assert call(matrix=None, oa=None, ob=None, ra=1024, rb=1025) == _lib.OK
        # an empty plane: zeros and NONE rows, and nothing else
        for hh, ww in ((0, 7), (6, 0), (0, 0)):
            d.poison(*OUTPUTS)
            assert call(hh=hh, ww=ww, pa=None, pb=None) == _lib.OK
            ctx.synchronize()
            got = read_outputs(d, 5, 5, OUTPUTS)
            assert (got["matrix"] == 0).all() and (got["counts"] == 0).all() and (got["a"] == [0, NONE, 0, 0]).all() and (got["b"] == [0, NONE, 0, 0]).all()
        d.poison(*OUTPUTS)
        assert call(hh=0, oa=None, matrix=None, counts=None) == _lib.OK and call(ia=300, flags=IGN_A) == _lib.OK  # (a u32 plane may ignore any u32)
        d.poison(*OUTPUTS)
        assert call(ra=3, rb=2) == _lib.OK
        ctx.synchronize()
        ref = reference(a.astype(np.uint32), b.astype(np.uint32), rows_a=3, rows_b=2)
        ga, gm = d.get("a").view(np.uint32), d.get("matrix").view(np.uint32)
        assert (ga[:12].reshape(3, 4) == ref.a).all() and (ga[12:] == 0xA5A5A5A5).all()  # rows beyond `rows` are the caller's
        assert (gm[:6].reshape(3, 2) == ref.matrix).all() and (gm[6:] == 0xA5A5A5A5).all()
    finally:
        d.free()
    # the host-pointer call: the same rules, outputs in host memory
    m, oa, ob, cn = np.full((5, 5), 9, np.uint32), np.full((5, 4), 9, np.uint32), np.full((5, 4), 9, np.uint32), np.full(8, 9, np.uint32)

    def host(ea=1, eb=1, flags=0, ia=0, ib=0, hh=6, ww=7, pa=a.ctypes.data, pb=b.ctypes.data, matrix=m.ctypes.data, ra=5, rb=5, slots=0):
        return L.infur_compare(h, pa, ea, pb, eb, hh, ww, flags, ia, ib, matrix, ra, rb, oa.ctypes.data, ob.ctypes.data, cn.ctypes.data, slots)

    assert host(ea=2) == host(eb=3) == host(flags=8) == host(ia=300) == host(ib=300) == host(pa=None) == host(pb=None) == host(slots=5) == bad
    assert host(hh=65536) == host(ww=65536) == host(ra=2048, rb=2048) == bad
    assert all((x == 9).all() for x in (m, oa, ob, cn))
    assert host() == _lib.OK
    ref = reference(a, b, rows_a=5, rows_b=5)
    assert (m == ref.matrix).all() and (oa == ref.a).all() and (ob == ref.b).all() and (cn == ref.counts).all()
    assert host(hh=0) == _lib.OK and (m == 0).all() and (cn == 0).all() and (oa == [0, NONE, 0, 0]).all()
    with pytest.raises(Exception):
        Compare(ctx).control(CompareCmd.Ignore(a=-1))


@pytest.mark.parametrize("ea,eb", ELEMS)
def test_host_pointer_call_and_processor(ctx, ea, eb):
    proc = Compare(ctx)
    assert proc.is_dirty()
    for (a, b), rows in (((R.smooth(135, 241), R.smooth(135, 241, seed=4)), (21, 21)), ((R.noise(33, 63, 21), R.noise(33, 63, 30)), (70, 70)),
                         ((CR.WORKED_A, CR.WORKED_B), (3, 3))):
        a, b = a.astype(ea), b.astype(eb)
        out = CompareOut(rows_a=rows[0], rows_b=rows[1])
        proc.control(CompareCmd.Ignore()).advance((a, b), out)
        ref = reference(a, b, rows_a=rows[0], rows_b=rows[1])
        assert not proc.is_dirty() and (out.matrix == ref.matrix).all() and (out.a == ref.a).all() and (out.b == ref.b).all() and (out.counts == ref.counts).all()
        ig = int(b[0, 0])
        proc.control(CompareCmd.Ignore(b=ig, pair_slots=64))
        assert proc.is_dirty()
        out = CompareOut(rows_a=rows[0], rows_b=rows[1], want_matrix=False)
        proc.advance((a, b), out)
        ref = reference(a, b, flags=IGN_B, ignore_b=ig, rows_a=rows[0], rows_b=rows[1], pair_slots=64)
        assert out.matrix is None and (out.a == ref.a).all() and (out.b == ref.b).all() and (out.counts == ref.counts).all()
    # the worked example of the header, word for word, and the measures a host makes of it
    out = CompareOut(rows_a=3, rows_b=3)
    Compare(ctx).advance((CR.WORKED_A.astype(ea), CR.WORKED_B.astype(eb)), out)
    assert out.matrix.tolist() == [[3, 0, 0], [1, 3, 0], [0, 1, 0]] and out.counts.tolist() == [8, 6, 0, 0, 4, 2, 6, 0]
    assert out.a.tolist() == [[3, 0, 3, 4], [4, 1, 3, 5], [1, 1, 1, 4]] and out.b.tolist() == [[4, 0, 3, 4], [4, 1, 3, 5], [0, NONE, 0, 0]]
    s = confusion_summary(out.matrix)
    assert s["pixel_accuracy"] == 0.75 and s["miou"] == pytest.approx(0.45)


# --------------------------------------------------------------------------- #
# 2. the fused frame path
# --------------------------------------------------------------------------- #
FRAME_H, FRAME_W = 96, 128


def truth_for(klass, seed=0):
    """a ground truth that agrees with most of the class plane: the plane shifted, with patches of "void" (255)"""
    t = CR.shifted(klass, 2, 3).copy()
    rng = np.random.default_rng(seed)
    for _ in range(4):
        y, x = int(rng.integers(0, t.shape[0] - 5)), int(rng.integers(0, t.shape[1] - 9))
        t[y:y + 5, x:x + 9] = 255
    return t


@pytest.mark.parametrize("decode", [RAW, SOFTMAX])
def test_fused_path_equals_segments_then_the_reference(ctx, model, decode):
    fp = FramePath(ctx)
    frame = W.synth_frame(FRAME_H, FRAME_W, index=5)
    for factor in (1.0, 0.5):
        s = fp.advance_segments(frame, factor, decode)
        truth = truth_for(s.klass)
        for ignore, flags in ((255, IGN_B), (None, 0)):
            ref = reference(s.klass, truth, flags=flags, ignore_b=ignore or 0, rows_a=21, rows_b=21)
            c = fp.advance_compare(frame, truth, factor, decode, ignore=ignore, want_klass=True, want_conf=True, want_scaled=True)
            assert (c.klass == s.klass).all() and (c.conf == s.conf).all() and c.scaled.shape == s.klass.shape + (3,)
            assert (c.matrix == ref.matrix).all() and (c.a == ref.a).all() and (c.b == ref.b).all() and (c.counts == ref.counts).all()
            q = fp.advance_compare(frame, truth, factor, decode, ignore=ignore, want_rows=False)  # the class plane goes to scratch
            assert q.klass is None and q.a is None and (q.matrix == ref.matrix).all() and (q.counts == ref.counts).all()
        assert ref.counts[CR.OUTSIDE] > 0 and ref.counts[CR.IGNORED] == 0  # 255 not ignored is a value above rows_b
        # the table form from the frame call
        t = fp.advance_compare(frame, truth, factor, decode, ignore=255, rows_a=64, rows_b=65, want_conf=True)
        ref = reference(s.klass, truth, flags=IGN_B, ignore_b=255, rows_a=64, rows_b=65)
        assert (t.matrix == ref.matrix).all() and (t.a == ref.a).all() and (t.b == ref.b).all() and (t.counts == ref.counts).all() and (t.conf == s.conf).all()
        acc = confusion_summary(c.matrix)
        assert 0.5 < acc["pixel_accuracy"] < 1.0 and 0.0 < acc["miou"] <= 1.0
        lo, _ = model.lowres()  # infur_model_read_lowres still works afterwards
        assert lo.size > 0 and np.isfinite(lo).all()


def test_fused_device_call_stays_inside_its_buffers(ctx, model):
    L, h = ctx.L, ctx.h
    hh, ww = FRAME_H, FRAME_W
    frame = W.synth_frame(hh, ww, index=2)
    s = FramePath(ctx).advance_segments(frame, 1.0, SOFTMAX)
    truth = truth_for(s.klass, seed=1)
    ref = reference(s.klass, truth, flags=IGN_B, ignore_b=255, rows_a=21, rows_b=23)
    d = Dev(ctx, bgr=frame.nbytes, truth=hh * ww, klass=hh * ww, conf=hh * ww, **out_sizes(21, 23))
    try:
        d.put("bgr", frame)
        d.put("truth", truth)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        P = d.ptr
        for want in (OUTPUTS, ("counts",), ("matrix", "klass"), ("a", "b", "conf"), ("counts", "klass", "conf")):
            d.poison("klass", "conf", *OUTPUTS)
            p = lambda name: P[name] if name in want else None  # noqa: E731
            ctx.check(L.infur_frame_compare_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, IGN_B, 255, P["truth"], hh * ww, p("klass"), p("conf"), hh * ww,
                                                p("matrix"), 21, 23, p("a"), p("b"), p("counts"), 0, None, C.byref(ow), C.byref(oh)))
            ctx.synchronize()
            assert (ow.value, oh.value) == (ww, hh)
            assert equal(read_outputs(d, 21, 23, want), ref, False)
            for name, plane in (("klass", s.klass), ("conf", s.conf)):
                got = d.get(name)
                assert (got.reshape(hh, ww) == plane).all() if name in want else (got == POISON).all(), (want, name)
            assert d.get("truth").tobytes() == truth.tobytes()
    finally:
        d.free()


def test_fused_rules_and_error_codes(ctx, model):
    L, h = ctx.L, ctx.h
    frame = W.synth_frame(48, 64, index=1)
    npix = 48 * 64
    s = FramePath(ctx).advance_segments(frame, 1.0, RAW)
    truth = truth_for(s.klass)
    m, oa, ob, cn = np.full((21, 21), 9, np.uint32), np.full((21, 4), 9, np.uint32), np.full((21, 4), 9, np.uint32), np.full(8, 9, np.uint32)
    klass = np.full((48, 64), 9, np.uint8)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    p = lambda x: x.ctypes.data if x is not None else None  # noqa: E731

    def call(lib=L, handle=h, decode=0, mode=0, factor=1.0, flags=IGN_B, ib=255, tr=truth, tr_cap=npix, kl=None, plane_cap=0, matrix=m, ra=21, rb=21,
             a=oa, b=ob, counts=cn, slots=0, scaled=None):
        return lib.infur_frame_compare(handle, p(frame), 64, 48, factor, mode, decode, flags, ib, p(tr), tr_cap, p(kl), None, plane_cap, p(matrix), ra, rb,
                                       p(a), p(b), p(counts), slots, p(scaled), C.byref(ow), C.byref(oh))

    assert call() == _lib.OK and (ow.value, oh.value) == (64, 48)
    ref = reference(s.klass, truth, flags=IGN_B, ignore_b=255, rows_a=21, rows_b=21)
    assert (m == ref.matrix).all() and (oa == ref.a).all() and (ob == ref.b).all() and (cn == ref.counts).all()
    assert call(decode=2) == _lib.E_INVALID_ARG and call(mode=2) != _lib.OK and call(factor=-1.0) == _lib.E_INVALID_SCALE
    assert call(flags=IGN_A) == _lib.E_INVALID_ARG and "only INFUR_COMPARE_IGNORE_B" in ctx.last_error()
    assert call(flags=4) == _lib.E_INVALID_ARG and call(ib=256) == _lib.E_INVALID_ARG and "ignore_b" in ctx.last_error()
    assert call(tr_cap=npix - 1) == _lib.E_CAPACITY and "truth plane" in ctx.last_error()
    assert call(tr=None) == _lib.E_INVALID_ARG and "truth" in ctx.last_error()
    assert call(kl=klass, plane_cap=npix - 1) == _lib.E_CAPACITY and (klass == 9).all()
    assert call(kl=klass, plane_cap=npix) == _lib.OK and (klass == s.klass).all()
    assert call(slots=3) == _lib.E_INVALID_ARG and "pair_slots" in ctx.last_error()
    assert call(matrix=None, a=None, b=None, counts=None) == _lib.E_INVALID_ARG and "no output wanted" in ctx.last_error()
    assert call(ra=2048, rb=2048, a=None, b=None) == _lib.E_INVALID_ARG and "2^20" in ctx.last_error()
    assert call(matrix=None, a=None, b=None) == _lib.OK and call(a=None, b=None, counts=None) == _lib.OK
    # no model: the Scale stage still runs, nothing else is produced
    with Context(device=0) as c:
        r = FramePath(c).advance_compare(frame, truth_for(np.zeros((24, 32), np.uint8)), 0.5, RAW, want_scaled=True, rows_a=21, rows_b=21)
        assert r.matrix is None and r.a is None and r.b is None and r.counts is None and r.klass is None and r.scaled.shape == (24, 32, 3)
        assert (r.scaled == FramePath(c).advance_segments(frame, 0.5, RAW, want_scaled=True).scaled).all()
        for x in (m, oa, ob, cn):
            x[:] = 9
        scaled = np.zeros((48, 64, 3), np.uint8)
        assert call(lib=c.L, handle=c.h, scaled=scaled) == _lib.E_MODEL_NOT_LOADED
        assert (scaled == FramePath(c).advance_segments(frame, 1.0, RAW, want_scaled=True).scaled).all()
        assert all((x == 9).all() for x in (m, oa, ob, cn))
        # a truth plane that is too short changes nothing about that: capacities are checked once a model is loaded
        assert call(lib=c.L, handle=c.h, tr_cap=3) == _lib.E_MODEL_NOT_LOADED


def test_regions_on_the_device_then_compare_on_the_device(ctx, model):
    """infur_frame_regions_dev, then infur_compare_dev of the label plane it left on the device against a ground-truth instance
    plane, INFUR_REGION_NONE ignored: per-object IoU and PQ, no dense plane to the host"""
    L, h = ctx.L, ctx.h
    hh, ww, rows = FRAME_H, FRAME_W, 512
    frame = W.synth_frame(hh, ww, index=3)
    r = FramePath(ctx).advance_regions(frame, 1.0, SOFTMAX, min_pixels=60, flags=_lib.REGIONS_SKIP_BACKGROUND, table_rows=rows)
    gt_labels, gt_table, gt_n = R.label(CR.shifted(r.klass, 1, 2), None, 8, min_pixels=60, flags=_lib.REGIONS_SKIP_BACKGROUND)
    assert 1 < r.n <= rows and 1 < gt_n <= rows and (r.labels == NONE).any()
    d = Dev(ctx, bgr=frame.nbytes, labels=hh * ww * 4, table=rows * 80, n=4, gt=hh * ww * 4, **out_sizes(rows, rows))
    try:
        P = d.ptr
        d.put("bgr", frame)
        d.put("gt", gt_labels)
        ow, oh = C.c_uint32(0), C.c_uint32(0)
        ctx.check(L.infur_frame_regions_dev(h, P["bgr"], ww, hh, 1.0, 0, SOFTMAX, 8, 60, _lib.REGIONS_SKIP_BACKGROUND, None, None, 0, P["labels"], hh * ww * 4,
                                            P["table"], rows, P["n"], None, C.byref(ow), C.byref(oh)))
        ctx.check(L.infur_compare_dev(h, P["labels"], 4, P["gt"], 4, hh, ww, IGN_A | IGN_B, NONE, NONE, None, rows, rows, P["a"], P["b"], P["counts"], 0))
        ctx.synchronize()
        got = read_outputs(d, rows, rows, ("a", "b", "counts"))
        ref = reference(r.labels, gt_labels, flags=IGN_A | IGN_B, ignore_a=NONE, ignore_b=NONE, rows_a=rows, rows_b=rows)
        assert equal(got, ref, True) and got["counts"][CR.MATCHED] > 0
        pq = panoptic_summary(got["a"], got["b"], list(r.table[:, _lib.REGION_CLASS]) + [0] * rows, list(gt_table[:, _lib.REGION_CLASS]) + [0] * rows)
        assert 0.0 < pq["pq"] <= 1.0 and sum(c["tp"] for c in pq["classes"].values()) <= got["counts"][CR.MATCHED]
    finally:
        d.free()


def test_compare_calls_leave_the_existing_legs_and_the_cached_graphs_alone(blob50):
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
        before = [fg.advance_regions(fr, 1.0, SOFTMAX) for fr in frames]  # the existing leg, before any Compare call on this context
        truth = R.smooth(120, 168, seed=1)
        for it in range(8):
            fr = frames[it % 4]
            rows = 65 if it & 2 else 21
            args = (fr, truth, 1.0, SOFTMAX if it & 1 else RAW)
            s = fg.advance_compare(*args, rows_a=64 if it & 2 else 21, rows_b=rows, want_klass=bool(it & 4), want_conf=bool(it & 4))
            e = fe.advance_compare(*args, rows_a=64 if it & 2 else 21, rows_b=rows)
            assert (s.matrix == e.matrix).all() and (s.a == e.a).all() and (s.b == e.b).all() and (s.counts == e.counts).all()
            a, _ = fe.advance(fr, 1.0)
            b, _ = fg.advance(fr, 1.0)
            assert (a == b).all(), it
        cap1, rep1, cached1 = cg.graph_stats()
        assert cap1 == cap0, "a compare call caused a capture"
        assert cached1 >= cached0, "a compare call dropped a cached graph"
        assert rep1 == rep0 + 8, "the frames between the compare calls were not replayed"
        for fr, b4 in zip(frames, before):  # and after: the same bytes
            now = fg.advance_regions(fr, 1.0, SOFTMAX)
            assert now.n == b4.n and all(getattr(now, f).tobytes() == getattr(b4, f).tobytes() for f in ("klass", "conf", "labels", "table"))


# --------------------------------------------------------------------------- #
# 3. the command line
# --------------------------------------------------------------------------- #
def test_cli_grades_every_frame_and_adds_the_matrices_up(tmp_path):
    import json
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames = [W.synth_frame(96, 128, index=i) for i in range(2)]
    (tmp_path / "clip.bgr24").write_bytes(b"".join(f.tobytes() for f in frames))
    base = [sys.executable, "-m", "infur_amd.segments_cli", "--width", "128", "--height", "96", "--synthetic-weights", "--softmax", "--input",
            str(tmp_path / "clip.bgr24")]
    r = subprocess.run(base + ["--labels-out", str(tmp_path / "klass.u8")], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = [json.loads(line) for line in r.stdout.splitlines()]
    klass = np.frombuffer((tmp_path / "klass.u8").read_bytes(), np.uint8).reshape(2, 96, 128)
    truth = np.stack([truth_for(k, seed=i) for i, k in enumerate(klass)])
    (tmp_path / "truth.u8").write_bytes(truth.tobytes())
    for extra in ([], ["--regions", "--max-regions", "64"]):
        r = subprocess.run(base + extra + ["--truth", str(tmp_path / "truth.u8"), "--truth-ignore", "255"], capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == 3 and lines[2]["frames"] == 2
        total = np.zeros((21, 21), np.uint64)
        for i in range(2):
            ref = reference(klass[i], truth[i], flags=IGN_B, ignore_b=255, rows_a=21, rows_b=21)
            want = confusion_summary(ref.matrix)
            assert lines[i]["pixel_accuracy"] == want["pixel_accuracy"] and lines[i]["miou"] == want["miou"]
            assert lines[i]["classes"] == plain[i]["classes"]  # what the line held before is unchanged
            total += ref.matrix
        want = confusion_summary(total)
        assert lines[2]["matrix"] == total.tolist() and lines[2]["miou"] == want["miou"] and lines[2]["pixel_accuracy"] == want["pixel_accuracy"]
        assert lines[2]["fwiou"] == want["fwiou"] and [c["klass"] for c in lines[2]["classes"]] == [c["klass"] for c in want["classes"] if c["union"]]
    short = subprocess.run(base + ["--truth", str(tmp_path / "klass.u8"), "--truth-ignore", "300"], capture_output=True, text=True, timeout=120, cwd=root)
    assert short.returncode != 0 and "--truth-ignore" in short.stderr
