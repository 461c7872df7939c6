"""tests/accuracy.py without a device: the readings on crafted arrays, the table against its own policy and against every scope the GPU
files ask for, the records (module docstring, LAB_NOTES.md) against the table, and the two planted faults of
tests/test_gpu_accuracy.py on an output whose error is 0."""
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import accuracy as A  # noqa: E402


# ---- readings ------------------------------------------------------------------------------------------------------------------------
def test_readings_on_arrays_with_known_answers():
    ref = np.array([[100.0, -50.0], [2.0, 0.5]])
    assert A.readings(ref, ref) == (0.0, 0.0, 0.0, 0.0)
    got = ref + np.array([[1.0, -1.0], [0.5, 0.25]])
    max_rel, elem, rms, bias = A.readings(got, ref)
    assert max_rel == pytest.approx(1.0 / 100.0)
    # 0.5 is not above 1e-2 x 100: its 50 % does not count; 2.0 is: 0.5 / 2.0
    assert elem == pytest.approx(0.25)
    ref_rms = math.sqrt((100.0 ** 2 + 50.0 ** 2 + 2.0 ** 2 + 0.5 ** 2) / 4)
    assert rms == pytest.approx(math.sqrt((1 + 1 + 0.25 + 0.0625) / 4) / ref_rms)
    assert bias == pytest.approx(abs(1.0 - 1.0 + 0.5 + 0.25) / 4 / ref_rms)
    # a constant offset is all bias: bias == rms; errors of alternating sign have none
    r = np.linspace(1.0, 2.0, 64)
    _, _, rms, bias = A.readings(r + 1e-3, r)
    assert bias == pytest.approx(rms)
    _, _, rms, bias = A.readings(r + 1e-3 * (-1.0) ** np.arange(64), r)
    assert bias < 1e-12 and rms > 1e-4
    # float32 inputs are widened before anything is subtracted
    a = np.float32(1.0) + np.float32(2.0 ** -23)
    assert A.readings(np.array([a], np.float32), np.array([1.0]))[0] == 2.0 ** -23
    # the wrappers are the first two readings
    import hostile as H

    assert H.errors(got, ref) == (max_rel, elem) and A.rel_err(got, ref) == max_rel and A.elem_err(got, ref) == elem


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_nan_and_inf_fail_every_reading(poison):
    ref = np.linspace(-1.0, 1.0, 33)
    got = ref.copy()
    got[7] = poison
    r = A.readings(got, ref)
    assert len(r) == 4
    for x in r:
        assert not x < math.inf  # the form every grader uses: `reading < bar`
    mode, scope = "f16", "hostile/layer"  # (the widest bars of the table)
    if (mode, scope) in A.MEASURED:
        assert A.failures(r, mode, scope) == list(A.NAMES)
        with pytest.raises(AssertionError):
            A.grade(got, ref, mode, scope, "poisoned")


def test_an_all_zero_reference_asserts():
    with pytest.raises(AssertionError):
        A.readings(np.ones(4), np.zeros(4))
    with pytest.raises(AssertionError):
        A.readings(np.ones(4), np.zeros(5))


def test_round_up_to_two_digits():
    assert A.round_up(1.3 * 1.07e-3) == 1.4e-3
    assert A.round_up(1.2e-5) == 1.2e-5 and A.round_up(1.2000001e-5) == 1.3e-5 and A.round_up(9.91e-4) == 1.0e-3
    for x in (3.3e-7, 0.123456, 5.0, 9.99e-3):
        assert x <= A.round_up(x) < x * 1.1


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def asked():
    return [(m, s) for s in A.SCOPES for m in A.ASKED[s]]


def test_every_mode_and_scope_a_gpu_test_asks_for_is_in_the_table():
    assert set(asked()) == set(A.MEASURED) == set(A.WAS)
    # the scopes the GPU files name as literals are the table's, and every scope is used by one of them
    used = set()
    for name in sorted(os.listdir(HERE)):
        if name.startswith("test_gpu_") and name.endswith(".py"):
            src = open(os.path.join(HERE, name)).read()
            if "A.grade(" not in src and "A.bar(" not in src:
                continue
            for scope in re.findall(r'"((?:hostile|friendly)/[a-z0-9]+|edge)"', src):
                assert scope in A.SCOPES, (name, scope)
                used.add(scope)
    # the own-error scopes are named by the classifier of tests/own_error.py (from the kernels that ran), through which
    # tests/test_gpu_own_error.py grades every layer
    import own_error as OE

    src = open(os.path.join(HERE, "test_gpu_own_error.py")).read()
    assert "OE.grade_own(" in src and "OE.assert_table(" in src
    assert set(OE.OWN_SCOPES) | set(OE.OWN16_SCOPES) == {s for s in A.SCOPES if s.startswith("own")}
    used |= set(OE.OWN_SCOPES) | set(OE.OWN16_SCOPES)
    # the rows of the own-error scopes at the derived cover sizes: tests/test_gpu_edge_cover.py grades a layer under cover/<kind> where
    # the (mode, kind) has such a row and under own/<kind> where it has none; every cover row stands beside an own row of its mode
    src = open(os.path.join(HERE, "test_gpu_edge_cover.py")).read()
    assert 'scope.replace("own", "cover", 1)' in src
    cover = {s for s in A.SCOPES if s.startswith("cover")}
    for s in cover:
        assert s.replace("cover", "own", 1) in A.SCOPES and set(A.ASKED[s]) <= set(A.ASKED[s.replace("cover", "own", 1)]), s
    used |= cover
    assert used == set(A.SCOPES)
    # the modes the files run under a scope (parametrize lists and loops) are spelled out in ASKED; the sweep's are the test's own
    src = open(os.path.join(HERE, "test_gpu_hostile.py")).read()
    assert 'SEED_MODES = ("f32", "f32s", "f32x", "f16hl")' in src and A.ASKED["hostile/seeds"] == ("f32", "f32s", "f32x", "f16hl")


def test_every_bar_is_the_policy_and_none_is_looser_than_before():
    for key in asked():
        meas, was, bars = A.MEASURED[key], A.WAS[key], A.bar(*key)
        assert len(meas) == len(was) == len(bars) == 4
        for x, w, b in zip(meas, was, bars):
            assert x > 0 and math.isfinite(x), key
            want = A.round_up(A.HEADROOM * x)
            assert A.HEADROOM * x <= want < A.HEADROOM * x * 1.1
            assert b == (want if w is None else min(w, want)), key
            assert w is None or b <= w, key
            assert x < b, (key, "the measured value itself misses the bar: a bar of before is tighter than the mode")
    assert A.HEADROOM == 1.3


# ---- the records ---------------------------------------------------------------------------------------------------------------------
def test_docstring_and_lab_notes_hold_the_table():
    notes = open(os.path.join(ROOT, "LAB_NOTES.md")).read()
    for line in A.table_lines():
        assert line in A.__doc__, line
        assert line in notes, line


def test_design_section_5_holds_the_own_error_rows():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("\n## 5. "):design.index("\n## 6. ")]
    lines = A.own_design_lines()
    assert len(lines) == sum(len(A.ASKED[s]) for s in A.SCOPES if s.startswith("own")) == 26
    for line in lines:
        assert line in sec, line
    assert "| mode | scope | measured: max_rel ; elem ; rms ; bias | bar (1.3 × measured) |" in sec
    # and no row of a (mode, scope) nobody asks for
    assert sum(1 for ln in sec.splitlines() if re.match(r"\| \w+ \| `own(16)?/", ln)) == len(lines)


def test_design_section_3_holds_the_tables_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("\n## 3. "):design.index("\n## 4. ")]
    header = [ln for ln in sec.splitlines() if ln.startswith("| mode (`INFUR_DTYPE_*`)")]
    assert len(header) == 1 and header[0].rstrip().endswith("| reading met (bar ≤ 1e-3) |") and "max_rel ; elem ; rms ; bias" in header[0]
    for mode, start in A.DESIGN_ROWS.items():
        rows = [ln for ln in sec.splitlines() if ln.startswith(start)]
        assert len(rows) == 1, (mode, len(rows))
        cells = [c.strip() for c in rows[0].strip().strip("|").split("|")]
        cell, met = A.design_cells(mode)
        assert cells[-2] == cell, (mode, cells[-2], cell)
        assert cells[-1] == met, (mode, cells[-1], met)
        # every number of the accuracy cell is a MEASURED value or a bar of the table
        nums = {f"{x:.1e}" for s in A.SCOPES if mode in A.ASKED[s] for t in (A.MEASURED[(mode, s)], A.bar(mode, s)) for x in t}
        assert set(re.findall(r"\d\.\de-\d\d", cells[-2])) <= nums
    # f32s per element: DESIGN states the bar it has, not the 1e-3 it does not hold
    assert A.design_cells("f32s")[1] == "max_rel" and A.design_cells("f32")[1] == "max_rel, elem"


# ---- the planted faults, on an output whose error is 0 ----------------------------------------------------------------------------------
def test_planted_faults_exceed_the_f32_edge_bars():
    from infur_amd import weights as W
    from oracle.infur_oracle import COracle, TorchModel

    h, w = 97, 61
    assert (h, w) in A.PLANT_SIZES
    blob = W.synth_blob()
    taps = {}
    lo, _ = TorchModel(blob, float64=True).forward_lowres(COracle().pack_normalize(W.synth_frame(h, w, index=h + w)), taps=taps)
    got, x = lo.numpy(), taps["classifier.0"].numpy()
    assert got.shape == (21, 13, 8) and x.shape == (512, 13, 8) and (13 * 8) % A.TAIL_TILE == 104
    wc, bc = A.classifier_of(blob)
    # the planting code recomputes the classifier the way the model does: unplanted, it gives the logits back
    exact = np.einsum("kc,chw->khw", wc, x) + bc[:, None, None]
    assert A.readings(exact, got)[0] < 1e-13
    assert A.readings(got, got) == (0.0, 0.0, 0.0, 0.0)
    p1 = A.readings(A.plant_p1(x, wc, bc), got)
    p2 = A.readings(A.plant_p2(got, x, wc), got)
    print(f"P1 on an exact output: {A.fmt(p1)}; P2: {A.fmt(p2)}; f32 edge bars {A.fmt(A.bar('f32', 'edge'))}")
    for name, r in (("P1", p1), ("P2", p2)):
        bad = A.failures(r, "f32", "edge")
        assert "max_rel" in bad and "rms" in bad, (name, r, bad)
    # what made the table necessary: the bars before it pass a half-precision classifier
    assert A.old_bars_pass(p1, "f32", "edge")
    # P2 touches the last 104 pixels only, all of this map; at 135x241 the last 15 of 527
    big = np.zeros((21, 17, 31))
    xs = np.ones((512, 17, 31))
    d = A.plant_p2(big, xs, np.ones((21, 512))) - big
    assert (d.reshape(21, -1)[:, :-15] == 0).all() and (d.reshape(21, -1)[:, -15:] == -32.0).all()
