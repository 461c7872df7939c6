"""Helper of tests/test_stage_limits_cpu.py and tests/test_gpu_stage_limits.py (a plain module like tests/edge_cover.py: no tests, no
product code): the SIZES at which the kernels of the decode stages change their walk, read off the sources, and the inputs that
cross them.

A stage kernel changes its walk where a trip count that depends on a declared row count or on the plane's size passes 1:

  grid-stride    a launch whose grid is capped deals its items (loops, arcs, wave-rows) round-robin to the waves of the grid,
                 `for (item = wave; item < n; item += waves)`.  A wave takes a second item only when the caller declares more rows
                 than the capped grid has waves AND the input holds more items than that
  scan-pass      one workgroup of kScanBlock lanes scans the block sums of a flag scan over rows + 1 positions (wave_scan.h:
                 scan_block_sums; coverage.hip: scan_sums64).  More than kScanBlock block sums -- more than kScanBlock^2 rows --
                 take a second pass of its loop, with the carry of the first
  counts-stride  one workgroup adds the block sums of the records launch, `for (k = threadIdx.x; k < NL; k += kScanBlock)`:
                 more than kScanBlock^2 loop rows give a lane a second term

Every cap is READ from the .hip text this tree carries (constant()): a cap that changes moves the cases or fails
tests/test_stage_limits_cpu.py, it never un-covers a kernel in silence.  The arithmetic of each launch is restated as a pure function
(waves, scan_passes, counts_strides, dense_trips) and held against a literal walk of the `for` by the CPU test.

REQUIRED names the crossings no test reached before this module, each with the case that crosses it; EXISTING names the test that
already reaches a crossing; OUT_OF_REACH lists what no input of a few seconds reaches, with the size it would take.  The survey
behind the three tables went through regions, tracks, runs, outlines, simplify, coverage, anchors, compare, sieve, shapes and the
Segments kernels of prepost.hip; a launch with one lane or one wave per element and a full grid has no such loop and is in no table.
"""
import functools
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "infur_amd", "csrc")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import compare_ref as CR  # noqa: E402
import coverage_ref as V  # noqa: E402
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import shapes_ref as H  # noqa: E402
import sieve_ref as A  # noqa: E402
import simplify_ref as S  # noqa: E402

WAVE = 64  # lanes of a wave on gfx950: every kernel below divides its workgroup by the literal 64


# ---- the caps, from the sources -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(source, name):
    """the value of `constexpr unsigned NAME = <digits>;` (or `constexpr int`) in infur_amd/csrc/<source>: exactly one match, else an
    error"""
    found = re.findall(r"constexpr (?:unsigned|int) " + re.escape(name) + r" = (\d+);", _text(source))
    if len(found) != 1:
        raise LookupError(f"{source}: {len(found)} definitions of {name}, expected exactly one")
    return int(found[0])


# (stage, kernel) -> (source, the constant of the grid's cap, the constant of the workgroup's lanes, the unit it deals)
LAUNCHES = {
    ("simplify", "simplify_keep_kernel"): ("simplify.hip", "kKeepGrid", "kKeepBlock", "loop"),
    ("shapes", "shapes_hull_kernel"): ("shapes.hip", "kLoopGrid", "kLoopBlock", "loop"),
    ("shapes", "shapes_rect_kernel"): ("shapes.hip", "kLoopGrid", "kLoopBlock", "loop"),
    ("coverage", "coverage_measure_kernel"): ("coverage.hip", "kWaveGrid", "kWaveBlock", "loop"),
    ("coverage", "coverage_emit_kernel"): ("coverage.hip", "kWaveGrid", "kWaveBlock", "loop"),
    ("coverage", "coverage_arcs_kernel"): ("coverage.hip", "kWaveGrid", "kWaveBlock", "arc"),
    ("compare", "compare_dense_kernel"): ("compare.hip", "kCmpDenseGrid", "kCmpBlock", "wave-row"),
}


def cap(stage, kernel):
    source, grid, _, _ = LAUNCHES[(stage, kernel)]
    return constant(source, grid)


def waves_per_block(stage, kernel):
    source, _, block, _ = LAUNCHES[(stage, kernel)]
    lanes = constant(source, block)
    assert lanes % WAVE == 0
    return lanes // WAVE


def scan_block():
    return constant("wave_scan.h", "kScanBlock")


# ---- the launches' arithmetic ---------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def grid_blocks(stage, kernel, rows):
    """the workgroups of the launch for `rows` declared rows (simplify.hip:296, shapes.hip:416-417, coverage.hip:612 wave_grid,
    compare.hip:304): min(ceil(rows / waves per workgroup), cap)"""
    return min(cdiv(rows, waves_per_block(stage, kernel)), cap(stage, kernel))


def waves(stage, kernel, rows):
    """the waves of the launch: every one walks `for (item = wave; item < n; item += waves)`"""
    return grid_blocks(stage, kernel, rows) * waves_per_block(stage, kernel)


def full_grid(stage, kernel):
    """the rows at which the grid reaches its cap: above them, and only there, a wave can meet a second item"""
    return cap(stage, kernel) * waves_per_block(stage, kernel)


def trips(stage, kernel, rows, n):
    """the largest number of items one wave of the launch takes when the input holds n"""
    w = waves(stage, kernel, rows)
    return cdiv(n, w) if w else 0


def scan_blocks(n):
    """wave_scan.h:15"""
    return cdiv(n, scan_block())


def scan_passes(rows):
    """passes of the loop of scan_block_sums (wave_scan.h:47) and scan_sums64 (coverage.hip:281) for a flag scan over the positions
    0 .. rows: NB = scan_blocks(rows + 1) block sums, kScanBlock a pass"""
    return cdiv(scan_blocks(rows + 1), scan_block())


def counts_strides(loops_rows):
    """terms one lane adds in simplify_counts_kernel (simplify.hip:236) and coverage_counts_kernel (coverage.hip:583): NL =
    scan_blocks(loops_rows) block sums of the records launch, kScanBlock lanes"""
    return cdiv(scan_blocks(loops_rows), scan_block())


def dense_trips(h, w):
    """wave-rows one wave of compare_dense_kernel walks (compare.hip:138): h * ceil(w / 64) of them on a grid of at most kCmpDenseGrid
    workgroups of four"""
    return cdiv(h * cdiv(w, WAVE), waves_per_block("compare", "compare_dense_kernel") * cap("compare", "compare_dense_kernel"))


def walk(blocks, per_block, n):
    """the `for` of a dealt launch, literally: for every (block, wave) pair the items it takes -> {(block, wave): [items]}"""
    total = blocks * per_block
    out = {}
    for b in range(blocks):
        for wv in range(per_block):
            items, item = [], b * per_block + wv
            while item < n:
                items.append(item)
                item += total
            out[(b, wv)] = items
    return out


# ---- the crossings --------------------------------------------------------------------------------------------------------------------
GRID, SCAN, COUNTS = "second trip of the grid-stride loop", "second pass of the block-sum scan", "second stride of the counts reduction"


def crossed(stage, kernel, crossing, rows=0, n=0, h=0, w=0):
    """does an input cross the line?  rows: the declared rows the launch's grid or scan comes from (loop rows; aug_rows for the arcs
    launch and Coverage's second scan; vertex rows for a vertex scan); n: the items the input holds (loops, arcs); h, w: Compare's plane"""
    if crossing == GRID and stage == "compare":
        # more than one tile a row below the cap's first stride: cmp_wave_row must split a strided u into row and tile
        return dense_trips(h, w) >= 2 and cdiv(w, WAVE) >= 2 and h >= 2
    if crossing == GRID:
        return rows > full_grid(stage, kernel) and n > waves(stage, kernel, rows) and trips(stage, kernel, rows, n) >= 2
    if crossing == SCAN:
        return scan_passes(rows) >= 2
    if crossing == COUNTS:
        return counts_strides(rows) >= 2
    raise ValueError(crossing)


# one row per (stage, kernel, crossing) that no test reached before tests/test_gpu_stage_limits.py: the rule it restates, the case
REQUIRED = (
    ("simplify", "simplify_keep_kernel", GRID, "simplify.hip:165 `loop += waves`, grid :296", "stacked"),
    ("shapes", "shapes_hull_kernel", GRID, "shapes.hip:234 `loop += waves`, grid :417", "stacked"),
    ("shapes", "shapes_rect_kernel", GRID, "shapes.hip:319 `loop += waves`, grid :417", "stacked"),
    ("coverage", "coverage_measure_kernel", GRID, "coverage.hip:204 `loop += waves`, grid :648", "stacked"),
    ("coverage", "coverage_emit_kernel", GRID, "coverage.hip:327 `loop += waves`, grid :653", "stacked"),
    ("coverage", "coverage_arcs_kernel", GRID, "coverage.hip:499 `k += waves`, grid :654 from aug_rows", "stacked"),
    ("shapes", "shapes_partials_kernel", SCAN, "shapes.hip:272 scan_block_sums over NB = scan_blocks(vertex_rows_in + 1), :415", "comb vertex rows"),
    ("coverage", "coverage_loop_partials_kernel", SCAN, "coverage.hip:281 scan_sums64 over NBL = scan_blocks(loops_rows_in + 1), :641", "smooth loop rows"),
    ("coverage", "coverage_partials_kernel", SCAN, "coverage.hip:536 scan_block_sums over NB = scan_blocks(aug_rows + 1), :641", "smooth aug rows"),
    ("simplify", "simplify_counts_kernel", COUNTS, "simplify.hip:236 `k += kScanBlock`, NL = scan_blocks(loops_rows_in), :291", "comb loop rows"),
    ("coverage", "coverage_counts_kernel", COUNTS, "coverage.hip:583 `k += kScanBlock`, NL = scan_blocks(loops_rows_in), :641", "smooth loop rows"),
    ("compare", "compare_dense_kernel", GRID, "compare.hip:138 `u += gridDim.x * 4` with tilesX > 1, grid :304", "compare tall"),
    ("sieve", "adj_scan_kernel", SCAN, "sieve.hip:267 scan_block_sums over scan_blocks(m.words), words = (2 x H x W + 31) / 32 of the bitmap of first edges, :86",
     "adjacency tall"),
)

# (stage, kernel, crossing, rule) -> "module::test" that reaches it.  Resolved by import in tests/test_stage_limits_cpu.py
EXISTING = (
    ("regions", "regions_scan_partials_kernel", SCAN, "regions.hip:179 scan_block_sums over H x W pixels", "test_gpu_regions::test_1080p_planes_equal_the_reference"),
    ("runs", "runs_partials_kernel", SCAN, "runs.hip:59 scan_block_sums over H x W pixels", "test_gpu_runs::test_more_than_1024_block_sums"),
    ("outlines", "outlines_edge_partials_kernel", SCAN, "outlines.hip:109 scan_block_sums over 4 x H x W edge slots",
     "test_gpu_outlines::test_more_than_1024_block_sums_single"),
    ("outlines", "outlines_loop_partials_kernel", SCAN, "outlines.hip:212-214 scan_block_sums over the edges, twice",
     "test_gpu_outlines::test_more_than_a_million_edges_checkerboard"),
    ("outlines", "outlines_round_kernel", "launches of the pointer-jumping round", "outlines.hip:306 `k < K`, K = ceil(log2(edge capacity))",
     "test_gpu_outlines::test_more_than_a_million_edges_checkerboard"),
    ("simplify", "simplify_partials_kernel", SCAN, "simplify.hip:183 scan_block_sums over NB = scan_blocks(vertex_rows_in + 1)",
     "test_gpu_simplify::test_comb_plane_one_long_loop_and_more_than_1024_block_sums"),
    ("simplify", "simplify_keep_kernel", "second stride of the lanes over a loop's vertices", "simplify.hip:93, :127 `i += 64u`",
     "test_gpu_simplify::test_wave_edges_on_the_stairs"),
    ("shapes", "shapes_hull_kernel", "second stride of the lanes over a loop's vertices", "shapes.hip:116, :155, :187 `+= 64u`",
     "test_gpu_shapes::test_hand_made_loops"),
    ("shapes", "shapes_rect_kernel", "second stride of the lanes over a hull's edges", "shapes.hip:327 `j += 64u`", "test_gpu_shapes::test_the_pinned_facts"),
    ("coverage", "coverage_measure_kernel", "second stride of the lanes over a loop's edges", "coverage.hip:209, :336 `+= 64u`",
     "test_gpu_coverage::test_planes_equal_the_reference"),
    ("anchors", "anchors_rows_kernel", "second tile of a wave, second tile of a lane", "anchors.hip:41, :80 `t += kAnchBlock / 64` (W > 256); :59 `t += kAnchBlock` (W > 16384)",
     "test_gpu_anchors::test_the_longest_sides"),
    ("compare", "compare_dense_kernel", "second trip of the grid-stride loop, one tile a row or one row", "compare.hip:138", "test_gpu_compare::test_the_longest_sides"),
    ("segments", "upsample_argmax_segments_kernel", "the scalar form in place of the staged one, by the plane's size",
     "prepost.hip:489 up_tile_lds_bytes: the staged footprint of tiny frames exceeds 48 KB; :643 `i += 256` over K * 8 words depends on the class count, not on a size",
     "test_gpu_decode_heads::test_every_class_count_at_every_size"),
    ("tracks", "tracks_scan_partials_kernel", "second scan block (one pass)", "tracks.hip:140 scan_block_sums over NB = scan_blocks(regions)",
     "test_gpu_tracks::test_the_new_track_scan_spans_several_blocks_with_ragged_ends"),
    ("tracks", "tracks_revive_choose_kernel", "second stride of the lanes over the gallery", "tracks.hip:276 `e += 64`",
     "test_gpu_tracks_memory::test_ragged4_crosses_scan_blocks_and_fills_the_gallery"),
)

# (stage, kernel, crossing, rule, the size it would take)
OUT_OF_REACH = (
    ("tracks", "tracks_scan_partials_kernel, tracks_mem_scan_partials_kernel", SCAN, "tracks.hip:140, :321 scan_block_sums over scan_blocks(min(rows, H x W, max regions))",
     "more than 2^20 regions in one frame, each with a table row: the shared scan_block_sums is executed by the rows above"),
    ("tracks", "tracks_gallery_partials_kernel", SCAN, "tracks.hip:410 scan_block_sums over scan_blocks(gallery rows + max regions)",
     "a gallery and a region capacity of more than 2^20 rows together"),
    ("simplify, shapes, coverage", "the records launches and every scan over loop rows with data beyond the first pass", SCAN + " with loops in it",
     "simplify.hip:206, coverage.hip:281", "more than 2^20 loops: the cases below declare the rows and leave the sums beyond the data zero"),
)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
SPARE = 5                # rows declared beyond the counts, as the dev_* helpers of the stage tests do
BIG_ROWS = 1100 * 1024   # more than kScanBlock^2: the row count of the scan and counts cases
STACK = dict(lattice_rows=356, width=372, band_rows=245, disc_r=120, hole_r=9, noise_cols=72, noise_classes=4, noise_seed=11)
COMPARE_SHAPE = (2100, 200)
ADJ = dict(width=4096, block=64, top_values=8, tail_rows=8, rows=16)  # Adjacency's plane: 2^24 pixels of blocks, then rows of new values


@functools.lru_cache(maxsize=None)
def stacked_plane():
    """(a): a lattice of isolated pixels (odd rows, odd columns, values cycling 1..3: one 4-vertex loop each) on top of a band of varied
    content: a disc with a round hole as value 2 beside regions_ref.noise.  Outlined with SKIP of value 0 and 4-connectivity.  Outlines numbers
    loops in START order, so the lattice fills the loop indices below the grid's waves and the band holds the ones beyond"""
    lat, w, band, r = STACK["lattice_rows"], STACK["width"], STACK["band_rows"], STACK["disc_r"]
    p = np.zeros((lat + band, w), np.uint8)
    ys, xs = np.arange(1, lat, 2), np.arange(1, w, 2)
    p[np.ix_(ys, xs)] = (np.arange(len(ys) * len(xs)) % 3 + 1).reshape(len(ys), len(xs))
    d = H.annulus(r, STACK["hole_r"]) * 2  # the disc of shapes_ref.disc(r) with a round hole: its outer loop is the disc's
    assert d.shape[0] + 1 <= band and d.shape[1] + STACK["noise_cols"] <= w
    p[lat + 1:lat + 1 + d.shape[0], :d.shape[1]] = d
    nz = R.noise(band, STACK["noise_cols"], STACK["noise_classes"], seed=STACK["noise_seed"])
    nz[0] = 0  # a row of the skipped value between the lattice and the band
    p[lat:, d.shape[1]:d.shape[1] + STACK["noise_cols"]] = nz
    p.setflags(write=False)
    return p


STACK_FLAGS, STACK_SKIP = O.SKIP, 0
VALUE_ROWS = 5  # per-value rows of Shapes on the stacked plane: the values 0..3 and one that stays empty


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def stacked_outline():
    return _frozen(O.outline(stacked_plane(), STACK_FLAGS, STACK_SKIP))


@functools.lru_cache(maxsize=None)
def stacked_simplify(tol16, loops_rows_in=None):
    l, v, c = stacked_outline()
    return _frozen(S.simplify(l, v, c, stacked_plane().shape[1], tol16, loops_rows_in=loops_rows_in))


@functools.lru_cache(maxsize=None)
def stacked_shapes(loops_rows_in=None):
    l, v, c = stacked_outline()
    return _frozen(H.shapes(l, v, c, stacked_plane().shape[1], rows=VALUE_ROWS, loops_rows_in=loops_rows_in))


@functools.lru_cache(maxsize=None)
def stacked_coverage(tol16):
    l, v, c = stacked_outline()
    return _frozen(V.coverage(stacked_plane(), l, v, c, tol16, V.SKIP, STACK_SKIP))


def stacked_aug_rows(vertex_rows):
    """what aug_rows = 0 stands for (infur_coverage.cpp:33-36): every declared vertex and every lattice vertex"""
    h, w = stacked_plane().shape
    return vertex_rows + (h + 1) * (w + 1)


@functools.lru_cache(maxsize=None)
def stacked_prefix(n_loops):
    """(b): the first n_loops loops of (a) as an input of its own: counts[0] the prefix length, counts[1] the end of its last loop"""
    l, v, c = stacked_outline()
    assert 0 < n_loops <= len(l)
    end = int(l[n_loops - 1, O.OFFSET]) + int(l[n_loops - 1, O.COUNT])
    return _frozen((l[:n_loops].copy(), v[:end].copy(), np.array([n_loops, end, 0], np.uint32)))


@functools.lru_cache(maxsize=None)
def prefix_simplify(n_loops, tol16):
    l, v, c = stacked_prefix(n_loops)
    return _frozen(S.simplify(l, v, c, stacked_plane().shape[1], tol16))


@functools.lru_cache(maxsize=None)
def prefix_shapes(n_loops):
    l, v, c = stacked_prefix(n_loops)
    return _frozen(H.shapes(l, v, c, stacked_plane().shape[1], rows=VALUE_ROWS))


def edge_prefixes(stage, kernel):
    """the loop counts just below, at and just above the waves of the capped grid"""
    full = full_grid(stage, kernel)
    return (full - 1, full, full + 1)


@functools.lru_cache(maxsize=None)
def comb_outline():
    """(c) for Simplify and Shapes: the comb of tests/test_gpu_simplify.py, one loop of more than 2^16 vertices"""
    plane = S.comb(130, 2100)
    return plane.shape, _frozen(O.outline(plane, O.SKIP, 0))


@functools.lru_cache(maxsize=None)
def comb_simplify(tol16):
    (h, w), (l, v, c) = comb_outline()
    return _frozen(S.simplify(l, v, c, w, tol16))


@functools.lru_cache(maxsize=None)
def comb_shapes():
    (h, w), (l, v, c) = comb_outline()
    return _frozen(H.shapes(l, v, c, w, rows=2))


@functools.lru_cache(maxsize=None)
def smooth_case(tol16=12):
    """(c) for Coverage: a smooth plane of its own, many loops and junctions in the first scan block"""
    k = R.smooth(65, 130)
    k.setflags(write=False)
    o = _frozen(O.outline(k))
    return k, o, _frozen(V.coverage(k, *o, tol16))


@functools.lru_cache(maxsize=None)
def compare_planes():
    """(d): four tiles a row and 8400 wave-rows"""
    h, w = COMPARE_SHAPE
    a, b = R.noise(h, w, 3, seed=h), R.smooth(h, w, seed=w)
    return a, b


def adjacency_words(h, w):
    """words of Adjacency's bitmap of first edge ids (sieve.hip:86): two edges a pixel, 32 a word"""
    return cdiv(2 * h * w, 32)


@functools.lru_cache(maxsize=None)
def adjacency_plane():
    """Adjacency's second pass: 64 x 64 blocks of the values 0..7 over the first 2^24 pixels -- every pair among them is first seen in
    the first pass of the scan -- and below them rows of noise over the values 8..15, whose pairs are first seen at edge ids beyond
    kScanBlock^2 words: their ranks need the carry of the first pass"""
    w, b = ADJ["width"], ADJ["block"]
    top_rows = cdiv(scan_block() * scan_block() * 32, 2 * w)  # the rows that fill the first pass: 4096 at this width
    blocks = R.noise(cdiv(top_rows, b), w // b, ADJ["top_values"], seed=3)
    top = np.kron(blocks, np.ones((b, b), np.uint8))[:top_rows]
    tail = R.noise(ADJ["tail_rows"], w, ADJ["rows"] - ADJ["top_values"], seed=4) + np.uint8(ADJ["top_values"])
    p = np.concatenate([top, tail]).astype(np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def adjacency_reference():
    p = adjacency_plane()
    return A.adjacency(p, ADJ["rows"], pair_rows=ADJ["rows"] * ADJ["rows"])


def case_numbers(case):
    """what a case declares and holds, from the references alone: {(stage, kernel, crossing): the arguments of crossed()}"""
    if case == "stacked":
        l, v, c = stacked_outline()
        nl, nv = int(c[0]), int(c[1])
        cov = stacked_coverage(16)[2]
        out = {(s, k, GRID): dict(rows=nl, n=nl) for (s, k), u in LAUNCHES.items() if u[3] == "loop"}  # the host-pointer entries declare the counts
        out[("coverage", "coverage_arcs_kernel", GRID)] = dict(rows=stacked_aug_rows(nv), n=int(cov[5]))
        return out
    if case == "comb vertex rows":
        return {("shapes", "shapes_partials_kernel", SCAN): dict(rows=BIG_ROWS)}
    if case == "comb loop rows":
        return {("simplify", "simplify_counts_kernel", COUNTS): dict(rows=BIG_ROWS)}
    if case == "smooth loop rows":
        return {("coverage", "coverage_loop_partials_kernel", SCAN): dict(rows=BIG_ROWS), ("coverage", "coverage_counts_kernel", COUNTS): dict(rows=BIG_ROWS)}
    if case == "smooth aug rows":
        return {("coverage", "coverage_partials_kernel", SCAN): dict(rows=BIG_ROWS)}
    if case == "adjacency tall":
        h, w = adjacency_plane().shape
        return {("sieve", "adj_scan_kernel", SCAN): dict(rows=adjacency_words(h, w) - 1)}  # (a scan over `words` positions: rows + 1 = words)
    if case == "compare tall":
        return {("compare", "compare_dense_kernel", GRID): dict(h=COMPARE_SHAPE[0], w=COMPARE_SHAPE[1])}
    raise KeyError(case)


def required_crossed(stage, kernel, crossing):
    """the REQUIRED row's own case crosses its line (tests/test_gpu_stage_limits.py asserts this before it runs the case)"""
    rows = [r for r in REQUIRED if r[:3] == (stage, kernel, crossing)]
    assert len(rows) == 1, (stage, kernel, crossing)
    return crossed(stage, kernel, crossing, **case_numbers(rows[0][4])[(stage, kernel, crossing)])


def tail_facts():
    """what the loops of (a) beyond the waves of the capped grid are like: the conditions tests/test_stage_limits_cpu.py holds them to"""
    l, v, c = stacked_outline()
    full = max(full_grid(s, k) for (s, k), u in LAUNCHES.items() if u[3] == "loop")
    tail = l[full:int(c[0])]
    lo, _, sh, _, _ = stacked_shapes()
    return dict(loops=len(tail), longer_than_4=int((tail[:, O.COUNT] > 4).sum()), longest=int(tail[:, O.COUNT].max()) if len(tail) else 0,
                largest_hull=int(lo[full:, H.COUNT].max()) if len(tail) else 0, holes=int((sh[full:, H.AREA2] < 0).sum()),
                values=len(set(tail[:, O.VALUE].tolist())))
