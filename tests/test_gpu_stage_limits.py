"""The polygon stages and Compare past the sizes at which their kernels change their walk (tests/stage_limits.py): a wave
of a capped grid takes a second loop or arc, the scan of the block sums takes a second pass, a lane of the counts reduction adds a
second term, Adjacency's bitmap scan takes a second pass, a wave of Compare's dense form walks a second wave-row of a plane with
several tiles a row.  Every case first asserts
from the table that it crosses its line -- a case that no longer crosses fails, it does not pass for nothing -- and then compares
whole arrays with ``==`` against the references: these stages are exact integers, there is no tolerance anywhere.  The buffers are
the poisoned, guard-padded ones of the stage tests, through their own helpers: what a call must leave alone still holds the poison,
and the inputs are unchanged.

On scratch builds: `loop += waves + 1` in shapes_hull_kernel and an `sp` that survives into a wave's next loop in
simplify_keep_kernel pass every older module of their stage and fail five tests each here; `carry = all` in coverage.hip's scan_sums64
passes the older modules and fails test_coverage_scans_take_a_second_pass[loops_rows_in].

Measured on an MI355X: 28 passed in 10.8 s, the slowest call 1.26 s (the first that needs Coverage's reference of the stacked plane)."""
import contextlib
import os
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd.processors import Context

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_ref as CR  # noqa: E402
import stage_limits as SL  # noqa: E402
import test_gpu_compare as TC  # noqa: E402  (check: Compare on poisoned buffers against its cached reference)
import test_gpu_coverage as TV  # noqa: E402  (dev_coverage, check_result)
import test_gpu_outlines as TO  # noqa: E402  (Dev: the poisoned, guard-padded device buffers)
import test_gpu_shapes as TH  # noqa: E402  (dev_shapes, check_result)
import test_gpu_sieve as TA  # noqa: E402  (dev_adjacency)
import test_gpu_simplify as TS  # noqa: E402  (dev_simplify, check_result)

pytestmark = pytest.mark.gpu

GRID, SCAN, COUNTS = SL.GRID, SL.SCAN, SL.COUNTS
POISON, POISON32 = TO.POISON, TO.POISON32
STAGES = ("simplify", "coverage", "shapes")
LOOP_KERNELS = {stage: [k for (s, k), u in SL.LAUNCHES.items() if s == stage and u[3] == "loop"] for stage in STAGES}
TOLS = {"simplify": (0, 16), "coverage": (16,), "shapes": (None,)}


def stacked():
    plane = SL.stacked_plane()
    l, v, c = SL.stacked_outline()
    return plane, l, v, c, int(c[0]), int(c[1])


def reference(stage, tol16):
    return SL.stacked_simplify(tol16) if stage == "simplify" else SL.stacked_coverage(tol16) if stage == "coverage" else SL.stacked_shapes()


def assert_crossed(stage, loops_rows, vertex_rows, n_loops):
    """the second trip of every dealt launch of the stage, under the rows this call declares"""
    for kernel in LOOP_KERNELS[stage]:
        assert SL.crossed(stage, kernel, GRID, rows=loops_rows, n=n_loops), (stage, kernel, loops_rows, n_loops)
    if stage == "coverage":
        n_arcs = int(SL.stacked_coverage(16)[2][5])
        assert SL.crossed(stage, "coverage_arcs_kernel", GRID, rows=SL.stacked_aug_rows(vertex_rows), n=n_arcs)


def dev_stage(ctx, stage, tol16, l, v, c, plane=None, **kw):
    """one stage through its device-pointer entry from host-built arrays, on its own module's poisoned buffers"""
    h, w = (plane if plane is not None else SL.stacked_plane()).shape
    if stage == "simplify":
        return TS.dev_simplify(ctx, l, v, c, h, w, tol16, **kw)
    if stage == "coverage":
        return TV.dev_coverage(ctx, plane if plane is not None else SL.stacked_plane(), l, v, c, tol16, SL.STACK_SKIP if plane is None else None, **kw)
    return TH.dev_shapes(ctx, l, v, c, h, w, rows=SL.VALUE_ROWS, **kw)


def check_stage(stage, ref, got, name=""):
    {"simplify": TS, "coverage": TV, "shapes": TH}[stage].check_result(ref, got, name)


def stage_bytes(stage, got):
    return [a.tobytes() for a in (got.values() if stage == "shapes" else got)]


# --------------------------------------------------------------------------- #
# (a) the stacked plane: 45 k loops, a quarter of them a wave's second
# --------------------------------------------------------------------------- #
@contextlib.contextmanager
def outlined_on_the_device(ctx, **outputs):
    """infur_outlines_dev on the stacked plane; lin, vin and cin stay in device memory for the stage that follows"""
    plane, l, v, c, nl, nv = stacked()
    h, w = plane.shape
    lrows, vrows = nl + 3, nv + 3
    d = TO.Dev(ctx, plane=plane.nbytes, lin=lrows * 16, vin=vrows * 4, cin=12, **outputs)
    try:
        d.put("plane", plane)
        P = d.ptr
        ctx.check(ctx.L.infur_outlines_dev(ctx.h, P["plane"], 1, h, w, SL.STACK_FLAGS, SL.STACK_SKIP, 0, P["lin"], lrows, P["vin"], vrows, P["cin"]))
        yield d, lrows, vrows

        ctx.synchronize()  # what Outlines left is what the reference says, and the stage left it alone
        assert d.get("cin").view(np.uint32).tolist() == c.tolist() and d.get("plane").tobytes() == plane.tobytes()
        lin, vin = d.get("lin").view(np.uint32).reshape(-1, 4), d.get("vin").view(np.uint32)
        assert (lin[:nl] == l).all() and (lin[nl:] == POISON32).all() and (vin[:nv] == v).all() and (vin[nv:] == POISON32).all()
    finally:
        d.free()


@pytest.mark.parametrize("stage", STAGES)
def test_stacked_plane_from_what_outlines_left_on_the_device(ctx, stage):
    plane, l, v, c, nl, nv = stacked()
    h, w = plane.shape
    arows = SL.stacked_aug_rows(nv + 3)
    sizes = dict(loops=(nl + 3) * 16, vertices=(arows if stage == "coverage" else nv + 3) * 4, counts=24 if stage == "coverage" else 16)
    if stage == "shapes":
        sizes.update(shapes=(nl + 3) * 96, values=SL.VALUE_ROWS * 96)
    with outlined_on_the_device(ctx, **sizes) as (d, lrows, vrows):
        assert_crossed(stage, lrows, vrows, nl)
        P, L = d.ptr, ctx.L
        for tol16 in TOLS[stage]:
            d.poison(*sizes)
            if stage == "simplify":
                ctx.check(L.infur_simplify_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], h, w, tol16, P["loops"], lrows, P["vertices"], vrows, P["counts"]))
            elif stage == "coverage":
                ctx.check(L.infur_coverage_dev(ctx.h, P["plane"], 1, h, w, _lib.COVERAGE_SKIP, SL.STACK_SKIP, P["lin"], lrows, P["vin"], vrows, P["cin"], tol16, 0,
                                               P["loops"], lrows, P["vertices"], arows, P["counts"]))
            else:
                ctx.check(L.infur_shapes_dev(ctx.h, P["lin"], lrows, P["vin"], vrows, P["cin"], h, w, P["loops"], lrows, P["vertices"], vrows, P["shapes"], lrows,
                                             P["values"], SL.VALUE_ROWS, P["counts"]))
            ctx.synchronize()
            loops, vertices, counts = d.get("loops").view(np.uint32).reshape(-1, 4), d.get("vertices").view(np.uint32), d.get("counts").view(np.uint32)
            if stage == "shapes":
                got = {"loops": loops, "vertices": vertices, "shapes": d.get("shapes").view(np.int64).reshape(-1, 12),
                       "values": d.get("values").view(np.int64).reshape(-1, 12), "counts": counts}
            else:
                got = (loops, vertices, counts)
            check_stage(stage, reference(stage, tol16), got, (stage, tol16))


@pytest.mark.parametrize("stage", STAGES)
def test_stacked_plane_from_host_built_arrays(ctx, stage):
    """the device-pointer entry on the module's own poisoned buffers, rows = counts + SPARE"""
    plane, l, v, c, nl, nv = stacked()
    assert_crossed(stage, nl + SL.SPARE, nv + SL.SPARE, nl)
    for tol16 in TOLS[stage]:
        ref = reference(stage, tol16)
        check_stage(stage, ref, dev_stage(ctx, stage, tol16, l, v, c, spare=SL.SPARE), (stage, tol16))
    if stage == "shapes":  # the 572-vertex disc is a wave's second loop, and its hull the rectangle launch's second lane stride
        full = SL.full_grid("shapes", "shapes_rect_kernel")
        disc = int(np.argmax(l[:, 1]))
        assert disc >= full and l[disc, 1] == 572 and ref[0][disc, 1] == 88 == ref[4][3] and (ref[2][full:, 0] < 0).any()


@pytest.mark.parametrize("stage", STAGES)
def test_stacked_plane_through_the_host_pointer_entry(ctx, stage):
    """the rows the device sees are the counts themselves: still more than the waves of the full grid"""
    plane, l, v, c, nl, nv = stacked()
    h, w = plane.shape
    assert_crossed(stage, nl, nv, nl)
    tol16 = TOLS[stage][-1]
    ref = reference(stage, tol16)
    li, vi, ci, pl = l.copy(), v.copy(), c.copy(), plane.copy()
    most = nv + (h + 1) * (w + 1) if stage == "coverage" else nv
    lo, vo = np.full((nl + 2, 4), POISON32, np.uint32), np.full(most + 2, POISON32, np.uint32)
    co = np.full(6 if stage == "coverage" else 4, POISON32, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    if stage == "simplify":
        ctx.check(ctx.L.infur_simplify(ctx.h, p(li), nl, p(vi), nv, p(ci), h, w, tol16, p(lo), nl + 2, p(vo), most + 2, p(co)))
        got = (lo, vo, co)
    elif stage == "coverage":
        ctx.check(ctx.L.infur_coverage(ctx.h, p(pl), 1, h, w, _lib.COVERAGE_SKIP, SL.STACK_SKIP, p(li), nl, p(vi), nv, p(ci), tol16, 0, p(lo), nl + 2, p(vo),
                                       most + 2, p(co)))
        got = (lo, vo, co)
    else:
        sh = np.full((nl + 2, 12), POISON, np.uint8).repeat(8, axis=1).view(np.int64)
        va = np.full((SL.VALUE_ROWS, 12), POISON, np.uint8).repeat(8, axis=1).view(np.int64)
        ctx.check(ctx.L.infur_shapes(ctx.h, p(li), nl, p(vi), nv, p(ci), h, w, p(lo), nl + 2, p(vo), most + 2, p(sh), nl + 2, p(va), SL.VALUE_ROWS, p(co)))
        got = {"loops": lo, "vertices": vo, "shapes": sh, "values": va, "counts": co}
    check_stage(stage, ref, got, stage)
    assert (li == l).all() and (vi == v).all() and (ci == c).all() and (pl == plane).all()  # the inputs are inputs


@pytest.mark.parametrize("stage", STAGES)
def test_stacked_plane_twice_in_one_context_and_once_in_a_second(ctx, stage):
    """identical bytes: the per-value rows of Shapes are built from atomicAdd and atomicMax of 45 k loops, which commute"""
    plane, l, v, c, nl, nv = stacked()
    assert_crossed(stage, nl + SL.SPARE, nv + SL.SPARE, nl)
    tol16 = TOLS[stage][-1]
    first = dev_stage(ctx, stage, tol16, l, v, c)
    k, (sl, sv, sc), _ = SL.smooth_case()
    small = dev_stage(ctx, stage, 12, sl, sv, sc, plane=k)  # a small call, another plane, in between
    again = dev_stage(ctx, stage, tol16, l, v, c)
    with Context(device=0) as c2:
        second_ctx = dev_stage(c2, stage, tol16, l, v, c)
    check_stage(stage, reference(stage, tol16), first, stage)
    for run in (again, second_ctx):
        assert stage_bytes(stage, run) == stage_bytes(stage, first)
    assert stage_bytes(stage, small) != stage_bytes(stage, first)


# --------------------------------------------------------------------------- #
# (b) Simplify and Shapes exactly at the edge: one loop fewer than, as many as and one more than the waves of the full grid
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("at", (-1, 0, 1))
@pytest.mark.parametrize("stage", ("simplify", "shapes"))
def test_loop_counts_around_the_waves_of_the_full_grid(ctx, stage, at):
    n = SL.full_grid(stage, LOOP_KERNELS[stage][0]) + at
    assert n in SL.edge_prefixes(stage, LOOP_KERNELS[stage][0])
    l, v, c = SL.stacked_prefix(n)
    assert c.tolist() == [n, int(l[-1, 0] + l[-1, 1]), 0]
    for kernel in LOOP_KERNELS[stage]:  # only the last wave-0 loop of the longest prefix is a second trip
        assert SL.crossed(stage, kernel, GRID, rows=n + SL.SPARE, n=n) == (at == 1)
        assert SL.trips(stage, kernel, n + SL.SPARE, n) == (2 if at == 1 else 1)
    # tolerance 0: a lattice square keeps its four corners, so a second trip that loses a vertex shows (at one pixel it keeps two)
    ref = SL.prefix_simplify(n, 0) if stage == "simplify" else SL.prefix_shapes(n)
    assert stage != "simplify" or (ref[0][:, 1] == 4).all()
    check_stage(stage, ref, dev_stage(ctx, stage, 0, l, v, c, spare=SL.SPARE), (stage, n))


@pytest.mark.parametrize("stage", ("simplify", "shapes"))
def test_the_full_list_under_the_rows_of_the_full_grid_is_truncated(ctx, stage):
    """the grid at its cap and more loops than rows: every wave sees no loop, the answer is the reference's truncated one"""
    plane, l, v, c, nl, nv = stacked()
    full = SL.full_grid(stage, LOOP_KERNELS[stage][0])
    assert nl > full == SL.waves(stage, LOOP_KERNELS[stage][0], full)
    ref = SL.stacked_simplify(16, full) if stage == "simplify" else SL.stacked_shapes(full)
    assert ref[-1].tolist() == ([nl, 0, 0, _lib.SIMPLIFY_TRUNCATED] if stage == "simplify" else [nl, 0, _lib.SHAPES_TRUNCATED, 0])
    got = dev_stage(ctx, stage, 16, l, v, c, loops_rows_in=full, loops_rows_out=nl, vertex_rows_out=nv)
    check_stage(stage, ref, got, stage)


# --------------------------------------------------------------------------- #
# (c) second passes of the block-sum scans, second strides of the counts reductions
# --------------------------------------------------------------------------- #
def test_shapes_vertex_scan_takes_a_second_pass(ctx):
    """The comb's one long loop under 1.1 M declared vertex rows.  The block sums beyond the data are zeros: what this checks is the
    carry into the total at partial[NB], the ranks of every kept vertex, and that the counts come out whole -- no more"""
    assert SL.required_crossed("shapes", "shapes_partials_kernel", SCAN)
    (h, w), (l, v, c) = SL.comb_outline()
    assert c[0] == 1 and c[1] > 1 << 16
    TH.check_result(SL.comb_shapes(), TH.dev_shapes(ctx, l, v, c, h, w, rows=2, vertex_rows_in=SL.BIG_ROWS), "vertex rows")


@pytest.mark.parametrize("stage", ("simplify", "shapes"))
def test_comb_under_more_than_a_million_loop_rows(ctx, stage):
    """1.1 M declared loop rows and one loop: Simplify's counts reduction gives each lane a second term (zeros beyond the data: the sums
    of the first stride must survive it, no more); the loop launches of both stages run on the full grid with one loop to find"""
    (h, w), (l, v, c) = SL.comb_outline()
    rows = SL.BIG_ROWS
    if stage == "simplify":
        assert SL.required_crossed("simplify", "simplify_counts_kernel", COUNTS) and SL.counts_strides(rows) >= 2
        for tol16 in (16, 65535):  # at 65535 the loop is degenerate: the count that the reduction carries is not zero
            ref = SL.comb_simplify(tol16)
            assert ref[2][2] == (tol16 == 65535)
            TS.check_result(ref, TS.dev_simplify(ctx, l, v, c, h, w, tol16, loops_rows_in=rows), tol16)
    else:
        assert SL.waves("shapes", "shapes_hull_kernel", rows) == SL.full_grid("shapes", "shapes_hull_kernel")
        TH.check_result(SL.comb_shapes(), TH.dev_shapes(ctx, l, v, c, h, w, rows=2, loops_rows_in=rows), "loop rows")


@pytest.mark.parametrize("which", ("loops_rows_in", "aug_rows"))
def test_coverage_scans_take_a_second_pass(ctx, which):
    """A smooth plane under 1.1 M declared loop rows (the 64-bit scan of coverage.hip and the counts reduction), then under 1.1 M
    augmented rows (the shared scan over the keep flags).  The sums beyond the data are zeros: what these check is the carry into the
    totals at part_n[NBL], part_a[NBL] and partial[NB], the offsets of every loop, and that the counts come out whole -- no more"""
    if which == "loops_rows_in":
        assert SL.required_crossed("coverage", "coverage_loop_partials_kernel", SCAN) and SL.required_crossed("coverage", "coverage_counts_kernel", COUNTS)
    else:
        assert SL.required_crossed("coverage", "coverage_partials_kernel", SCAN)
    k, (l, v, c), ref = SL.smooth_case()
    assert ref[2][2] > 0 and ref[2][4] > len(v) and ref[2][5] > len(l)  # degenerate loops, junctions and arcs for the totals to carry
    TV.check_result(ref, TV.dev_coverage(ctx, k, l, v, c, 12, **{which: SL.BIG_ROWS}), which)


def test_adjacency_bitmap_scan_takes_a_second_pass(ctx):
    """Adjacency ranks its pair records by the first edge id, through a bitmap of two bits a pixel: beyond 2^24 pixels the scan of the
    bitmap's block sums takes a second pass, and here 28 of the 120 pairs are first seen there: their ranks need the carry"""
    assert SL.required_crossed("sieve", "adj_scan_kernel", SCAN)
    plane, ref, rows = SL.adjacency_plane(), SL.adjacency_reference(), SL.ADJ["rows"]
    n, beyond = len(ref.pairs), 32 * SL.scan_block() ** 2
    assert n == rows * (rows - 1) // 2 and (ref.pairs[:, 3] >= beyond).sum() >= rows and ref.counts[7] == 0  # every pair, no overflow
    got = TA.dev_adjacency(ctx, plane, rows, pair_rows=rows * rows)
    assert (got["counts"] == ref.counts).all(), (got["counts"], ref.counts)
    assert (got["rows"] == ref.rows).all()
    assert (got["pairs"][:n] == ref.pairs).all() and (got["pairs"][n:].view(np.uint8) == POISON).all()


# --------------------------------------------------------------------------- #
# (d) Compare's dense form past its cap with four tiles a row
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("eb", (np.uint8, np.uint32))
def test_compare_dense_form_strides_over_rows_and_tiles(ctx, eb):
    assert SL.required_crossed("compare", "compare_dense_kernel", GRID)
    a, b = SL.compare_planes()
    h, w = a.shape
    assert SL.crossed("compare", "compare_dense_kernel", GRID, h=h, w=w) and SL.dense_trips(h, w) == 2 and -(-w // 64) == 4
    b = b.astype(eb)
    ref = TC.check(ctx, a, b, "tall", rows_a=21, rows_b=21)
    assert ref.counts[CR.STATUS] == 0 and ref.counts[CR.OUTSIDE] == 0 and ref.counts[CR.COMPARED] == h * w and ref.counts[CR.RUNS] > h * 4
    table = TC.check(ctx, a, b, "tall, the table form as the control", rows_a=64, rows_b=65)  # one wave-row a wave: no stride
    assert table.counts[CR.STATUS] == CR.TABLE and (table.counts[:7] == ref.counts[:7]).all()
    assert (table.matrix[:21, :21] == ref.matrix).all() and table.matrix.sum() == ref.matrix.sum()
