"""tests/stage_limits.py without a GPU: the caps are read from the sources, every restated launch rule equals a literal walk of the
kernel's `for`, every REQUIRED crossing is crossed by its case on the references' own counts, the loops of the stacked plane beyond
the capped grid are varied, every reference answers in seconds, and every EXISTING row names a test that exists."""
import importlib
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_limits as SL  # noqa: E402

GRID_LAUNCHES = sorted(SL.LAUNCHES)
STAGE_SOURCES = ("regions.hip", "tracks.hip", "runs.hip", "outlines.hip", "simplify.hip", "coverage.hip", "anchors.hip", "compare.hip", "sieve.hip",
                 "shapes.hip", "prepost.hip")


# ---- the constants ----------------------------------------------------------------------------------------------------------------------
def test_every_cap_is_read_from_the_sources_exactly_once():
    for (stage, kernel), (source, grid, block, _) in SL.LAUNCHES.items():
        assert SL.constant(source, grid) > 0 and SL.constant(source, block) % SL.WAVE == 0, (stage, kernel)
        assert f"{kernel}" in SL._text(source), (kernel, source)  # the kernel the row names is in the file the row names
    assert SL.scan_block() > 0 and SL.scan_block() % SL.WAVE == 0
    # the stage kernels divide their workgroups by the literal 64 this module calls WAVE
    for source, block in {(u[0], u[2]) for u in SL.LAUNCHES.values()}:
        assert re.search(re.escape(block) + r" / 64\b", SL._text(source)) or block == "kCmpBlock", (source, block)
    assert "gridDim.x * 4" in SL._text("compare.hip") and SL.waves_per_block("compare", "compare_dense_kernel") == 4


def test_a_missing_or_doubled_constant_is_an_error(monkeypatch):
    with pytest.raises(LookupError):
        SL.constant("shapes.hip", "kNoSuchGrid")
    text = SL._text("shapes.hip")
    monkeypatch.setattr(SL, "_text", lambda name: text + "\nconstexpr unsigned kLoopGrid = 4096;\n")
    with pytest.raises(LookupError):
        SL.constant("shapes.hip", "kLoopGrid")
    monkeypatch.setattr(SL, "_text", lambda name: text.replace("constexpr unsigned kLoopGrid = ", "constexpr unsigned kLoopGrid = 2 * "))
    with pytest.raises(LookupError):  # not a plain number any more: no silent default
        SL.constant("shapes.hip", "kLoopGrid")


def test_a_changed_cap_moves_the_rule(monkeypatch):
    read = SL._text
    old = SL.cap("shapes", "shapes_hull_kernel")
    monkeypatch.setattr(SL, "_text", lambda name: read(name).replace(f"kLoopGrid = {old};", f"kLoopGrid = {4 * old};"))
    assert SL.cap("shapes", "shapes_hull_kernel") == 4 * old and SL.full_grid("shapes", "shapes_hull_kernel") == 16 * old
    nl = int(SL.stacked_outline()[2][0])
    assert not SL.crossed("shapes", "shapes_hull_kernel", SL.GRID, rows=nl, n=nl)  # the case no longer crosses: the tests below would fail


def test_the_survey_names_files_that_are_there():
    for source in STAGE_SOURCES:
        assert SL._text(source)
    for row in SL.REQUIRED + SL.EXISTING + SL.OUT_OF_REACH:
        for source in re.findall(r"(\w+\.(?:hip|h)):\d+", row[3]):
            assert os.path.exists(os.path.join(SL.CSRC, source)), row
    for stage, kernel, _, rule, _ in SL.REQUIRED:
        source = re.match(r"(\w+\.hip):", rule).group(1)
        assert kernel in SL._text(source), (kernel, source)
        for line in re.findall(source.replace(".", r"\.") + r":(\d+)", rule):  # the line the rule cites holds the loop or the call it names
            assert re.search(r"for \(|scan_block_sums|scan_sums64", SL._text(source).splitlines()[int(line) - 1]), (rule, line)


# ---- the restated rules against the kernels' loops, walked literally ------------------------------------------------------------------
def rows_around(*centres, spread=40):
    out = set(range(0, 12))
    for c in centres:
        out |= set(range(max(c - spread, 0), c + spread + 1))
    return sorted(out)


@pytest.mark.parametrize("stage,kernel", GRID_LAUNCHES)
def test_waves_and_trips_equal_the_walk(monkeypatch, stage, kernel):
    """a small cap in place of the source's (the walk of 32 Ki waves for hundreds of row counts would take minutes): the rule is the same
    function of the cap"""
    source, grid, block, _ = SL.LAUNCHES[(stage, kernel)]
    per = SL.waves_per_block(stage, kernel)
    real = SL.constant
    for small in (1, 7, 32):
        monkeypatch.setattr(SL, "constant", lambda s, n, small=small: small if (s, n) == (source, grid) else real(s, n))
        full = small * per
        for rows in rows_around(full, 2 * full, spread=2 * per + 3):
            blocks = min(-(-rows // per), small)  # the launch line, literally
            assert SL.grid_blocks(stage, kernel, rows) == blocks and SL.waves(stage, kernel, rows) == blocks * per
            for n in sorted({0, 1, rows // 2, rows - 1, rows, rows + 1, full - 1, full, full + 1, 2 * full, 2 * full + 1, 3 * full + 5} - {-1}):
                if rows == 0:
                    continue  # (no launch)
                taken = SL.walk(blocks, per, n)
                assert sorted(i for items in taken.values() for i in items) == list(range(n))  # every item once
                most = max(len(items) for items in taken.values())
                assert SL.trips(stage, kernel, rows, n) == most, (small, rows, n)
                if stage != "compare" and n <= rows:  # (counts above the rows are truncated input: the kernels see no item)
                    assert SL.crossed(stage, kernel, SL.GRID, rows=rows, n=n) == (most >= 2), (small, rows, n)
    monkeypatch.setattr(SL, "constant", real)
    # at the source's own cap: the closed form at the three loop counts of the edge case
    full = SL.full_grid(stage, kernel)
    assert [SL.trips(stage, kernel, full + 9, n) for n in (full - 1, full, full + 1)] == [1, 1, 2]
    assert SL.waves(stage, kernel, full + 9) == full == SL.waves(stage, kernel, full) and SL.waves(stage, kernel, full - per) == full - per


def test_a_wave_meets_a_second_item_only_with_rows_and_items_beyond_the_full_grid():
    for stage, kernel in GRID_LAUNCHES:
        if stage == "compare":
            continue
        full = SL.full_grid(stage, kernel)
        assert not SL.crossed(stage, kernel, SL.GRID, rows=full, n=full)          # the grid at its cap, every wave one item
        assert not SL.crossed(stage, kernel, SL.GRID, rows=2 * full, n=full)      # rows beyond it, the items not
        assert SL.crossed(stage, kernel, SL.GRID, rows=full + 1, n=full + 1)
        assert SL.trips(stage, kernel, full, 2 * full) == 2  # (a caller whose counts exceed the rows is truncated: the kernels see no loop)


def test_scan_passes_and_counts_strides_equal_the_walk():
    B = SL.scan_block()
    for rows in rows_around(B - 1, B * B - 1, B * B, 2 * B * B - 1, spread=3) + [SL.BIG_ROWS]:
        nb = len(range(0, rows + 1, B))  # blocks of the sums launch over the positions 0 .. rows
        assert SL.scan_blocks(rows + 1) == nb
        assert SL.scan_passes(rows) == len(range(0, nb, B))  # `for (base = 0; base < NB; base += kScanBlock)`
        nl = -(-rows // B)
        strides = max((len(range(t, nl, B)) for t in (0, B - 1)), default=0)  # `for (k = threadIdx.x; k < NL; k += kScanBlock)`
        assert SL.counts_strides(rows) == strides, rows
    assert SL.scan_passes(B * B - 1) == 1 and SL.scan_passes(B * B) == 2          # rows + 1 positions
    assert SL.counts_strides(B * B) == 1 and SL.counts_strides(B * B + 1) == 2
    assert SL.scan_passes(SL.BIG_ROWS) == 2 == SL.counts_strides(SL.BIG_ROWS)


def test_dense_trips_equal_the_walk(monkeypatch):
    real = SL.constant
    for small in (1, 5):
        monkeypatch.setattr(SL, "constant", lambda s, n, small=small: small if n == "kCmpDenseGrid" else real(s, n))
        for h in range(1, 40):
            for w in (1, 64, 65, 200, 300):
                wave_rows = h * -(-w // 64)
                blocks = min(-(-wave_rows // 4), small)
                most = max(len(items) for items in SL.walk(blocks, 4, wave_rows).values())
                assert SL.dense_trips(h, w) == most, (small, h, w)
    monkeypatch.setattr(SL, "constant", real)
    assert SL.dense_trips(1, 65535) == 1 and SL.dense_trips(65535, 1) == 8  # the longest sides: the cap is crossed by rows of one tile only
    assert not SL.crossed("compare", "compare_dense_kernel", SL.GRID, h=65535, w=1) and not SL.crossed("compare", "compare_dense_kernel", SL.GRID, h=1, w=65535)
    assert not SL.crossed("compare", "compare_dense_kernel", SL.GRID, h=135, w=241) and not SL.crossed("compare", "compare_dense_kernel", SL.GRID, h=2, w=16500)


# ---- the cases cross their lines, on the references alone ------------------------------------------------------------------------------
def test_every_size_dependent_launch_has_a_row():
    assert {(r[0], r[1]) for r in SL.REQUIRED if r[2] == SL.GRID} == set(SL.LAUNCHES)
    assert len({r[:3] for r in SL.REQUIRED}) == len(SL.REQUIRED)
    assert {r[2] for r in SL.REQUIRED} == {SL.GRID, SL.SCAN, SL.COUNTS}
    for stage in ("regions", "tracks", "runs", "outlines", "simplify", "coverage", "anchors", "compare", "sieve", "shapes", "segments"):
        assert any(stage in r[0] for r in SL.REQUIRED + SL.EXISTING + SL.OUT_OF_REACH), stage
    assert all(len(r) == 5 and r[4] for r in SL.OUT_OF_REACH)  # each says the size it would take


@pytest.mark.parametrize("row", SL.REQUIRED, ids=lambda r: f"{r[1]}-{r[2].split()[1]}")
def test_required_crossings_are_crossed(row):
    stage, kernel, crossing, _, case = row
    numbers = SL.case_numbers(case)[(stage, kernel, crossing)]
    assert SL.crossed(stage, kernel, crossing, **numbers), (row, numbers)
    assert SL.required_crossed(stage, kernel, crossing)
    if crossing == SL.GRID and stage != "compare":
        assert numbers["rows"] > SL.full_grid(stage, kernel) and numbers["n"] > SL.waves(stage, kernel, numbers["rows"])
    elif crossing == SL.GRID:
        assert SL.dense_trips(**numbers) >= 2
    elif crossing == SL.SCAN:
        assert SL.scan_passes(numbers["rows"]) >= 2
    else:
        assert SL.counts_strides(numbers["rows"]) >= 2


def test_the_stacked_plane_is_what_the_cases_take_it_for():
    l, v, c = SL.stacked_outline()
    nl, nv = int(c[0]), int(c[1])
    assert (l[1:nl, 3].astype("int64") > l[:nl - 1, 3].astype("int64")).all()  # START strictly increasing: the lattice comes first
    full = SL.full_grid("shapes", "shapes_hull_kernel")
    assert all(SL.full_grid(s, k) == full for (s, k), u in SL.LAUNCHES.items() if u[3] != "wave-row")
    assert (l[:full, 1] == 4).all()  # below the waves of the grid: the lattice, one pixel a loop
    # every way the GPU test declares rows: the counts themselves (host-pointer entries), + 3 (what Outlines left), + SPARE
    for spare in (0, 3, SL.SPARE):
        for (stage, kernel), u in SL.LAUNCHES.items():
            if u[3] == "loop":
                assert SL.crossed(stage, kernel, SL.GRID, rows=nl + spare, n=nl)
        assert SL.crossed("coverage", "coverage_arcs_kernel", SL.GRID, rows=SL.stacked_aug_rows(nv + spare), n=int(SL.stacked_coverage(16)[2][5]))
    # the edge prefixes, and the full list under the rows of the full grid: truncated
    assert SL.edge_prefixes("simplify", "simplify_keep_kernel") == (full - 1, full, full + 1) == SL.edge_prefixes("shapes", "shapes_rect_kernel")
    for n in (full - 1, full, full + 1):
        pl, pv, pc = SL.stacked_prefix(n)
        assert pc.tolist() == [n, 4 * n, 0] and len(pl) == n and len(pv) == 4 * n
        assert SL.crossed("simplify", "simplify_keep_kernel", SL.GRID, rows=n + SL.SPARE, n=n) == (n == full + 1)
    assert SL.stacked_simplify(16, full)[2].tolist() == [nl, 0, 0, 1] and SL.stacked_shapes(full)[4].tolist() == [nl, 0, 1, 0]


def test_the_loops_beyond_the_grid_are_varied():
    """conditions, not measurements: the second trip of a wave must meet loops that differ from one another"""
    t = SL.tail_facts()
    print(t)
    assert t["loops"] >= 2000
    assert t["longer_than_4"] >= 500
    assert t["longest"] > 128
    assert t["largest_hull"] > 64  # the rectangle kernel's second lane stride, on a wave's second loop
    assert t["holes"] >= 1
    assert t["values"] >= 3


TIMED = """
import json, sys, time
sys.path.insert(0, sys.argv[1])
import stage_limits as SL
full = SL.full_grid("simplify", "simplify_keep_kernel")
timed = (("outline", SL.stacked_outline, ()), ("simplify 0", SL.stacked_simplify, (0,)), ("simplify 16", SL.stacked_simplify, (16,)),
         ("shapes", SL.stacked_shapes, ()), ("coverage 16", SL.stacked_coverage, (16,)), ("comb outline", SL.comb_outline, ()),
         ("comb simplify", SL.comb_simplify, (16,)), ("comb shapes", SL.comb_shapes, ()), ("smooth coverage", SL.smooth_case, ()),
         ("prefix simplify", SL.prefix_simplify, (full + 1, 0)), ("prefix shapes", SL.prefix_shapes, (full + 1,)),
         ("adjacency", SL.adjacency_reference, ()), ("compare", lambda: SL.CR.compare(*SL.compare_planes(), rows_a=21, rows_b=21), ()))
SL.stacked_plane(), SL.adjacency_plane(), SL.compare_planes()
out = {}
for name, fn, args in timed:
    for _ in range(5):  # the smallest of up to five readings: a busy machine adds time, it never takes any away
        if name != "outline":
            SL.stacked_outline()
        if hasattr(fn, "cache_clear"):
            fn.cache_clear()
        w0, c0 = time.perf_counter(), time.process_time()
        fn(*args)
        wall, cpu = time.perf_counter() - w0, time.process_time() - c0
        out[name] = min(out.get(name, 1e9), wall, cpu)
        if out[name] < 3.0:
            break
print("TIMES " + json.dumps(out))
"""


def test_every_reference_answers_in_seconds():
    """Each reference on its first call, in an interpreter of its own, so that the reading is the reference's and not the state a
    long pytest session leaves behind; the smaller of the wall clock and the process's CPU seconds, so that it is not the machine's
    other work either (these references are single-threaded: on a quiet machine the two agree)"""
    r = subprocess.run([sys.executable, "-c", TIMED, SL.HERE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    times = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")][0][6:])
    print(times)
    assert len(times) == 13
    for name, seconds in times.items():
        assert seconds < 3.0, (name, seconds)


# ---- the tests EXISTING names ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SL.EXISTING, ids=lambda r: r[4].split("::")[1][:40])
def test_existing_rows_name_tests_that_exist(row):
    module, name = row[4].split("::")
    mod = importlib.import_module(module)
    fn = getattr(mod, name)  # a typo fails here
    assert callable(fn) and name.startswith("test_")
    assert os.path.dirname(os.path.abspath(mod.__file__)) == SL.HERE
    marks = getattr(mod, "pytestmark", None)
    assert marks is not None and "gpu" in str(marks)  # the crossing is reached on the device
