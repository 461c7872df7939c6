"""The walks of tests/stage_history.py, checked without a GPU, on the references alone: the poisons are poisons.  "All equal" in
tests/test_gpu_stage_history.py must not be able to mean "nothing was at stake" -- a BIG plane that is no larger in some count, a
SAME-DENSE plane that gives the target's answer, a STOPPED call that runs to its end, a sparse plane whose answer is not empty.
The conditions are fixed; if a seed breaks one, the seed changes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import compare_ref as CR  # noqa: E402
import runs_ref as U  # noqa: E402
import stage_history as SH  # noqa: E402
import tracks_memory_ref as M  # noqa: E402
import tracks_ref as T  # noqa: E402

COUNTS = ("regions", "runs", "n_loops", "n_vertices", "n_edges", "kept", "n_aug", "n_arcs", "pairs", "compare_runs")
shape_id = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def test_the_table_is_the_one_the_suite_documents():
    assert SH.SHAPES == [(33, 65), (7, 65), (2, 130), (1, 5)] and SH.BIG == (136, 248)
    assert SH.STAGES == ("segments", "regions", "tracks", "runs", "outlines", "simplify", "coverage", "anchors", "compare")
    assert set(SH.PLANE_STAGES) | {"segments", "tracks"} == set(SH.STAGES)
    for stage in SH.PLANE_STAGES:
        ts = SH.targets(stage)
        assert {t.shape for t in ts} == set(SH.SHAPES) and {t.content for t in ts} == {"moderate", "dense"}
        assert {t.elem for t in ts} == ({1} if stage == "regions" else {1, 4})
        assert len(ts) == len(set(ts)) == 4 * 2 * len(SH.elems_of(stage)) * (2 if stage == "compare" else 1)
    # Regions' target consults the per-root pixel counts: with min_pixels 0 or 1 they are never read
    assert all(SH.args(SH.target_call("regions", t))["min_pixels"] == 3 for t in SH.targets("regions"))
    # Anchors' rows lie above the number of values
    assert all(SH.args(SH.target_call("anchors", t))["rows"] > 21 for t in SH.targets("anchors"))


@pytest.mark.parametrize("shape", SH.SHAPES, ids=shape_id)
def test_big_and_same_dense_exceed_the_moderate_target_in_every_count(shape):
    mod, den, big, near = SH.counts(SH.moderate(shape)), SH.counts(SH.dense(shape)), SH.counts(SH.big()), SH.counts(SH.near(shape))
    assert sorted(mod) == sorted(COUNTS)
    print(f"{shape}: moderate {mod}\n dense {den}\n BIG {big}")
    for name in COUNTS:
        assert big[name] > mod[name], ("BIG", name)
        assert den[name] > mod[name], ("SAME-DENSE", name)
        assert big[name] >= den[name] and near[name] > mod[name], name  # BIG is no smaller than the dense target either
    assert SH.BIG[0] > shape[0] + 1 and SH.BIG[1] > shape[1] + 1  # larger than the target, and than NEAR, in both sides
    p = SH.near(shape)
    assert (p.h, p.w) == (shape[0] + 1, shape[1] + 1)


def test_the_counts_of_33x65_are_the_documented_ones():
    mod, den = SH.counts(SH.moderate((33, 65))), SH.counts(SH.dense((33, 65)))
    assert [mod[k] for k in ("regions", "runs", "n_loops", "n_vertices", "n_edges")] == [122, 550, 131, 1334, 2262]
    assert [den[k] for k in ("regions", "runs", "n_loops", "n_vertices", "n_edges")] == [1762, 2052, 1945, 7824, 8180]


@pytest.mark.parametrize("shape", SH.SHAPES, ids=shape_id)
def test_the_dense_target_exceeds_same_sparse_whose_answer_is_empty(shape):
    den = SH.counts(SH.dense(shape))
    for zero in (False, True):  # (Regions can skip class 0 only: its sparse plane holds that)
        sp = SH.counts(SH.sparse(shape, zero=zero), skip=True)
        for name in ("regions",) if zero else COUNTS[1:]:
            assert sp[name] == 0 < den[name], (zero, name)
    # ... and the calls the walks make say so themselves: no region, no run, no loop, no kept vertex, no distance, no pair
    for stage in SH.PLANE_STAGES:
        for t in SH.targets(stage):
            if t.shape != shape or t.content != "dense":
                continue
            (pc,) = [c for name, c, _ in SH.walk_steps(stage, t) if name == "SAME-SPARSE"]
            assert (pc.plane.h, pc.plane.w, pc.plane.elem) == (shape[0], shape[1], t.elem)
            exp = SH.expected(pc)
            if stage == "regions":
                assert exp["n"][0] == 0 and (exp["labels"] == 0xFFFFFFFF).all()
            elif stage == "runs":
                assert exp["n"][0] == 0 and (exp["row_start"] == 0).all()
            elif stage == "outlines":
                assert exp["counts"].tolist() == [0, 0, 0]
            elif stage == "simplify":
                assert exp["counts"].tolist() == [0, 0, 0, 0]
            elif stage == "coverage":
                assert exp["counts"].tolist() == [0, 0, 0, 0, 0, 0]
            elif stage == "anchors":
                assert (exp["dist2"] == 0).all() and (exp["anchors"] == [0xFFFFFFFF, 0]).all()
            else:
                c = exp["counts"]
                assert c[CR.COMPARED] == 0 == c[CR.PAIRS] == c[CR.RUNS] and c[CR.IGNORED] == shape[0] * shape[1] and (exp["matrix"] == 0).all()
            assert not any(name == "SAME-DENSE" for name, _, _ in SH.walk_steps(stage, t))


@pytest.mark.parametrize("stage", SH.PLANE_STAGES)
def test_same_dense_differs_from_the_target_in_every_output(stage):
    seen = 0
    for t in SH.targets(stage):
        if t.content != "moderate":
            continue
        steps = SH.walk_steps(stage, t)
        (pc,) = [c for name, c, _ in steps if name == "SAME-DENSE"]
        tc = steps[0][2]
        assert (pc.plane.h, pc.plane.w, pc.plane.elem) == (t.shape[0], t.shape[1], t.elem) and pc.plane.kind == "dense"
        want, stale = SH.expected(tc), SH.expected(pc)
        assert list(want) == list(stale)
        for name in want:
            a, b = want[name], stale[name]
            common = tuple(slice(0, min(m, n)) for m, n in zip(a.shape, b.shape))  # (the rows move with the counts and with the
            a, b = a[common], b[common]  # poison's declared rows: the common block is where stale data would show)
            k = a.size
            if stage == "anchors" and name == "dist2" and t.shape[0] <= 2:
                # a plane of one or two rows: every pixel touches the frame and has distance 1, whatever the plane holds.  So
                # SAME-DENSE is no poison for dist2 at (2, 130) and (1, 5): there the other poisons and `anchors` carry the walk
                assert (a == 1).all() and (b == 1).all()
                continue
            assert k > 0 and (a != b).any(), (SH.tag(tc), name)
        seen += 1
    assert seen == 4 * len(SH.elems_of(stage)) * (2 if stage == "compare" else 1)


def test_every_stopped_call_really_stops():
    stopped = {stage: [c for name, c, _ in SH.walk_steps(stage, SH.targets(stage)[0]) if name == "STOPPED"] for stage in SH.PLANE_STAGES}
    assert {s: len(v) for s, v in stopped.items()} == {"regions": 1, "runs": 1, "outlines": 1, "simplify": 1, "coverage": 2, "anchors": 0, "compare": 1}
    assert all(c.plane == SH.big() for v in stopped.values() for c in v)
    big = SH.counts(SH.big())
    # Regions, Runs: n above the rows
    exp, a = SH.expected(stopped["regions"][0]), SH.args(stopped["regions"][0])
    assert 0 < a["rows"] < exp["n"][0]
    exp, a = SH.expected(stopped["runs"][0]), SH.args(stopped["runs"][0])
    assert 0 < a["rows"] < exp["n"][0] == big["runs"]
    # Outlines: {0, 0, n_edges}, nothing else written
    exp, a = SH.expected(stopped["outlines"][0]), SH.args(stopped["outlines"][0])
    assert a["max_edges"] == big["n_edges"] - 1 and exp["counts"].tolist() == [0, 0, big["n_edges"]]
    assert (exp["loops"].view(np.uint8) == SH.POISON).all() and (exp["vertices"].view(np.uint8) == SH.POISON).all()
    # Simplify, Coverage: status 1 with one loop row short; Coverage: status 4 with one augmented row short
    exp, a = SH.expected(stopped["simplify"][0]), SH.args(stopped["simplify"][0])
    assert a["loops_rows_in"] == big["n_loops"] - 1 and exp["counts"].tolist() == [big["n_loops"], 0, 0, 1]
    exp, a = SH.expected(stopped["coverage"][0]), SH.args(stopped["coverage"][0])
    assert a["loops_rows_in"] == big["n_loops"] - 1 and exp["counts"].tolist() == [big["n_loops"], 0, 0, 1, 0, 0]
    exp, a = SH.expected(stopped["coverage"][1]), SH.args(stopped["coverage"][1])
    assert a["aug_rows"] == big["n_aug"] - 1 and exp["counts"].tolist() == [big["n_loops"], 0, 0, 4, big["n_aug"], 0]
    # Compare: the table form, OVERFLOW
    exp, a = SH.expected(stopped["compare"][0]), SH.args(stopped["compare"][0])
    assert not CR.is_dense(a["rows_a"], a["rows_b"]) and a["pair_slots"] == 64
    assert exp["counts"][CR.STATUS] == CR.TABLE | CR.OVERFLOW and exp["counts"][CR.PAIRS] == 0 and 2 * exp["counts"][CR.RUNS] > 64


def test_compare_forms_are_on_the_sides_the_rule_says():
    assert CR.is_dense(*SH.DENSE_ROWS) and not CR.is_dense(*SH.TABLE_ROWS)
    for t in SH.targets("compare"):
        a = SH.args(SH.target_call("compare", t))
        assert CR.is_dense(a["rows_a"], a["rows_b"]) == (t.form == "dense")
        assert bool(SH.expected(SH.target_call("compare", t))["counts"][CR.STATUS] & CR.TABLE) == (t.form == "table")
        others = [SH.args(c) for name, c, _ in SH.walk_steps("compare", t) if name == "OTHER-FORM"]
        assert any(CR.is_dense(o["rows_a"], o["rows_b"]) != (t.form == "dense") for o in others)
        # the table is walked with 64 slots and with the default
        slots = {o["pair_slots"] for o in others if not CR.is_dense(o["rows_a"], o["rows_b"])} | ({a["pair_slots"]} if t.form == "table" else set())
        assert slots == {0, 64}


def test_the_u32_planes_hold_none_and_values_a_float_would_round():
    t = U.u32_table()
    assert t[0] == 0xFFFFFFFF and (t > (1 << 24)).sum() > 200
    for shape in SH.SHAPES:
        for p in (SH.moderate(shape, 4), SH.dense(shape, 4)):
            plane = SH.plane_of(p)
            assert plane.dtype == np.uint32 and (plane == t[SH.plane_of(p._replace(elem=1))]).all()
            assert plane.max() > (1 << 24)
    # 0xFFFFFFFF stands for class 0.  The planes' seeds are fixed, and three small planes hold no class 0: both 1x5 planes (five
    # pixels) and the moderate 2x130 plane.  Every other target plane, and BIG, holds it.
    holds = {(p.kind, p.h, p.w): bool((SH.plane_of(p) == 0xFFFFFFFF).any()) for shape in SH.SHAPES for p in (SH.moderate(shape, 4), SH.dense(shape, 4))}
    assert [k for k, v in holds.items() if not v] == [("moderate", 2, 130), ("moderate", 1, 5), ("dense", 1, 5)]
    assert holds[("moderate", 33, 65)] and holds[("moderate", 7, 65)] and holds[("dense", 33, 65)] and holds[("dense", 7, 65)] and holds[("dense", 2, 130)]
    assert (SH.plane_of(SH.big(4)) == 0xFFFFFFFF).any()


@pytest.mark.parametrize("stage", SH.PLANE_STAGES)
def test_every_walk_has_every_poison_the_stage_defines(stage):
    for t in SH.targets(stage):
        steps = SH.walk_steps(stage, t)
        names = [name for name, _, _ in steps]
        want = {"BIG", "NEAR", "SAME-DENSE" if t.content == "moderate" else "SAME-SPARSE", "OTHER-FORM", "REJECTED"}
        want |= {"OTHER-ELEM"} if stage in SH.TAKES_ELEM else set()
        want |= {"STOPPED"} if stage != "anchors" else set()
        want |= {"EMPTY"} if stage != "coverage" else set()  # (Coverage refuses an empty plane: its h and w start at 1)
        assert set(names) == want, (stage, t)
        tc = SH.target_call(stage, t)
        assert all(c == tc for _, _, c in steps) and all(pc != tc and pc.stage == stage for _, pc, _ in steps)
        assert len({pc for _, pc, _ in steps}) == len(steps)
        for name, pc, _ in steps:
            assert (pc.expect != "OK") == (name == "REJECTED")
            a = SH.args(pc)
            if name == "BIG":
                assert (pc.plane.h, pc.plane.w) == SH.BIG
            if name == "OTHER-ELEM":
                assert pc.plane == tc.plane._replace(elem=5 - t.elem)
            if name == "EMPTY":
                assert pc.plane.h * pc.plane.w == 0
            # the host staging moves with the rows: the poisons of another plane, and of the same one in the other element size,
            # declare other rows than the target
            for key in ("rows", "loops_rows", "loops_rows_in", "loops_rows_out", "rows_a", "rows_b"):
                if key in a and name in ("BIG", "NEAR", "SAME-DENSE", "SAME-SPARSE", "OTHER-ELEM", "STOPPED"):
                    assert a[key] != SH.args(tc)[key], (SH.tag(pc), key)
            if stage == "compare" and name in ("BIG", "NEAR", "SAME-DENSE", "SAME-SPARSE", "OTHER-ELEM"):  # the target's own form
                assert CR.is_dense(a["rows_a"], a["rows_b"]) == (t.form == "dense")
        if stage == "anchors":
            # Anchors' rows size the keys' memset and move dist2 in the host staging (256-byte steps: above 32 rows): poisons above
            # that step and one below the target's rows
            rows = {name: SH.args(pc)["rows"] for name, pc, _ in steps if name != "REJECTED"}
            assert SH.args(tc)["rows"] * 8 <= 256 < min(rows["BIG"], rows["OTHER-ELEM"], rows["OTHER-FORM"]) * 8 and rows["NEAR"] < SH.args(tc)["rows"]


def test_the_tracks_walk():
    case = SH.tracks_case()
    import walks

    assert all(case.h * case.w <= c.h * c.w for c in walks.CASES) and case.max_lost > 0
    seq = SH.tracks_sequence()
    assert len(seq) == 4 and all(labels.shape == (case.h, case.w) and rows > n > 0 for labels, _, n, rows in seq)
    steps = SH.tracks_reference()
    assert sum(int(s.summary[T.CONTINUED]) for s in steps) > 0 and all(s.memory is not None for s in steps)
    # the poisoning handle: three BIG steps, the gallery overfull, far more regions and gallery rows than the sequence ever has
    ref, big = SH.tracks_poisoned_reference()
    assert len(big) == 3 and big[-1].summary[T.STATUS] & M.GALLERY_FULL and big[-1].memory[M.HELD] == SH.TRACK_BIG_GALLERY
    assert min(n for _, _, n in SH.tracks_big_frames()) > 100 * max(n for _, _, n, _ in seq)
    assert all(labels.shape == SH.BIG for labels, _, _ in SH.tracks_big_frames())
    # the reused handle: reset and memory off and on forget everything but the frame counter
    ref.reset(0)
    ref.set_memory(0)
    ref.set_memory(case.max_lost, case.reach, case.gallery_rows)
    for a, b in zip(SH.tracks_reference(ref), steps):
        later = b.table.copy()
        later[later[:, T.ID] != T.NONE, T.BORN] += SH.TRACK_BIG_STEPS
        assert (a.table == later).all() and (a.track_of_region == b.track_of_region).all() and (a.plane == b.plane).all()
        assert a.summary.tolist() == b.summary.tolist() and a.memory.tolist() == b.memory.tolist() and (a.gap_of_region == b.gap_of_region).all()
        held = b.gallery.copy()
        held[:, (M.L_BORN, M.L_SEEN)] += SH.TRACK_BIG_STEPS
        assert (a.gallery == held).all()


def test_the_segments_walk():
    ts = SH.segments_targets()
    assert {(k, h, w) for k, h, w, _, _ in ts} == {(k, h, w) for k in (3, 21) for h, w in ((7, 65), (33, 65))} and {d for _, _, _, d, _ in ts} == {0, 1}
    for t in ts:
        k, h, w, decode, seed = t
        ps = dict(SH.segments_poisons(t))
        assert ps["LARGER-K"][0] > k and ps["LARGER-K"][1:3] == (h, w)
        assert ps["BIG"][0] == k and ps["BIG"][1] > h and ps["BIG"][2] > w
        assert ps["SAME"][:4] == (k, h, w, decode) and ps["OTHER-FORM"][:4] == (k, h, w, 1 - decode)
        x, y = SH.logits(k, h, w, seed), SH.logits(*ps["SAME"][:3], ps["SAME"][4])
        assert (x.argmax(axis=0) != y.argmax(axis=0)).mean() > 0.3  # other content: another class plane


def test_first_difference_names_output_count_and_index():
    a = {"labels": np.zeros((2, 3), np.uint32), "n": np.array([4], np.uint32), "empty": np.zeros((0, 4), np.uint32)}
    b = {k: v.copy() for k, v in a.items()}
    assert SH.first_difference(a, b) is None
    b["labels"][1, 2] = 7
    b["labels"][0, 1] = 9
    msg = SH.first_difference(a, b)
    assert msg.startswith("labels: 2 of 6") and "(0, 1)" in msg and "9" in msg
    b["labels"][:] = 0
    b["n"][0] = 5
    assert SH.first_difference(a, b).startswith("n: 1 of 1")
    assert "missing" in SH.first_difference(a, {"labels": a["labels"]})
    assert "against" in SH.first_difference({"n": np.zeros(2, np.uint32)}, {"n": np.zeros(3, np.uint32)})
