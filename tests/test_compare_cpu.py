"""Compare (the confusion matrix and the best partner per value between two planes) without a GPU: the ABI surface, the reference
the GPU tests use (tests/compare_ref.py) against a brute-force double loop and np.bincount, the header's worked example word for
word, the reference's own identities, and the two host helpers of infur_amd.processors on hand-worked cases."""
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd.processors import confusion_summary, panoptic_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_ref as CR  # noqa: E402
import regions_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_compare", "infur_compare_dev", "infur_frame_compare", "infur_frame_compare_dev")
CONSTANTS = {"INFUR_COMPARE_IGNORE_A": 1, "INFUR_COMPARE_IGNORE_B": 2, "INFUR_COMPARE_PIXELS": 0, "INFUR_COMPARE_PARTNER": 1, "INFUR_COMPARE_INTER": 2,
             "INFUR_COMPARE_UNION": 3, "INFUR_COMPARE_WORDS": 4, "INFUR_COMPARE_COMPARED": 0, "INFUR_COMPARE_EQUAL": 1, "INFUR_COMPARE_IGNORED": 2,
             "INFUR_COMPARE_OUTSIDE": 3, "INFUR_COMPARE_PAIRS": 4, "INFUR_COMPARE_MATCHED": 5, "INFUR_COMPARE_RUNS": 6, "INFUR_COMPARE_STATUS": 7,
             "INFUR_COMPARE_COUNT_WORDS": 8, "INFUR_COMPARE_OVERFLOW": 1, "INFUR_COMPARE_TABLE": 2, "INFUR_FEATURE_COMPARE": 512}
NONE = CR.NONE
SMALL = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (2, 130), (13, 70))


def pairs_of(h, w):
    yield "smooth/shifted", R.smooth(h, w, seed=h + w, classes=5, cell=4), CR.shifted(R.smooth(h, w, seed=h + w, classes=5, cell=4), min(1, h - 1), min(2, w - 1))
    yield "noise2/noise3", R.noise(h, w, 2, seed=w), R.noise(h, w, 3, seed=h)
    yield "identical", R.noise(h, w, 4, seed=1), R.noise(h, w, 4, seed=1)
    yield "single/noise", R.single(h, w), R.noise(h, w, 5, seed=2)


def settings():
    yield dict(rows_a=5, rows_b=5)
    yield dict(rows_a=2, rows_b=3)  # some pixels outside
    yield dict(rows_a=5, rows_b=5, flags=CR.IGNORE_A, ignore_a=1)
    yield dict(rows_a=5, rows_b=4, flags=CR.IGNORE_B, ignore_b=0)
    yield dict(rows_a=4, rows_b=5, flags=CR.IGNORE_A | CR.IGNORE_B, ignore_a=3, ignore_b=1)
    yield dict(rows_a=70, rows_b=70)  # the table form's status
    yield dict(rows_a=0, rows_b=5)


def same(x, y):
    return (x.matrix == y.matrix).all() and (x.a == y.a).all() and (x.b == y.b).all() and (x.counts == y.counts).all()


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_COMPARE
    assert _lib.FEATURE_COMPARE == 512 and lib.infur_features() & 511 == 511  # the nine older bits stay set
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version


def test_constants_agree_in_the_header_python_rust_and_the_reference():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, value in CONSTANTS.items():
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rust), name
        assert getattr(_lib, name[len("INFUR_"):]) == value, name
    assert "#define INFUR_COMPARE_NONE 0xFFFFFFFFu" in header and _lib.COMPARE_NONE == NONE
    assert (CR.IGNORE_A, CR.IGNORE_B, CR.WORDS, CR.COUNT_WORDS, CR.OVERFLOW, CR.TABLE) == (1, 2, 4, 8, 1, 2)
    assert (CR.PIXELS, CR.PARTNER, CR.INTER, CR.UNION) == (_lib.COMPARE_PIXELS, _lib.COMPARE_PARTNER, _lib.COMPARE_INTER, _lib.COMPARE_UNION)
    assert [CR.COMPARED, CR.EQUAL, CR.IGNORED, CR.OUTSIDE, CR.PAIRS, CR.MATCHED, CR.RUNS, CR.STATUS] == list(range(8))


def test_rejected_calls_need_no_gpu(lib):
    b = np.full(16, 0x5A5A5A5A, np.uint32)
    p = b.ctypes.data
    assert lib.infur_compare(None, p, 1, p, 1, 2, 2, 0, 0, 0, p, 1, 1, p, p, p, 0) == _lib.E_INVALID_ARG
    assert lib.infur_compare_dev(None, p, 1, p, 1, 2, 2, 0, 0, 0, p, 1, 1, p, p, p, 0) == _lib.E_INVALID_ARG
    assert (b == 0x5A5A5A5A).all()


def test_the_worked_example_word_for_word():
    r = CR.compare(CR.WORKED_A, CR.WORKED_B, rows_a=3, rows_b=3)
    assert r.matrix.tolist() == [[3, 0, 0], [1, 3, 0], [0, 1, 0]]
    assert r.a.tolist() == [[3, 0, 3, 4], [4, 1, 3, 5], [1, 1, 1, 4]]
    assert r.b.tolist() == [[4, 0, 3, 4], [4, 1, 3, 5], [0, NONE, 0, 0]]
    assert r.counts.tolist() == [8, 6, 0, 0, 4, 2, 6, 0]  # COMPARED EQUAL IGNORED OUTSIDE PAIRS MATCHED RUNS STATUS
    s = confusion_summary(r.matrix, names=["a", "b", "c"])
    assert s["pixel_accuracy"] == 6 / 8 and [c["iou"] for c in s["classes"]] == [3 / 4, 3 / 5, 0.0]
    assert s["miou"] == pytest.approx(0.45, abs=1e-15)
    # with rows_a = 2 the pixel with a = 2 is outside
    r = CR.compare(CR.WORKED_A, CR.WORKED_B, rows_a=2, rows_b=3)
    assert r.counts[CR.OUTSIDE] == 1 and r.matrix.shape == (2, 3) and r.b[1, CR.PIXELS] == 3
    assert same(r, CR.brute(CR.WORKED_A, CR.WORKED_B, rows_a=2, rows_b=3))


def test_reference_equals_the_brute_force_double_loop():
    n = 0
    for h, w in SMALL:
        for name, a, b in pairs_of(h, w):
            for kw in settings():
                for ea, eb in ((np.uint8, np.uint8), (np.uint32, np.uint8)):
                    assert same(CR.compare(a.astype(ea), b.astype(eb), **kw), CR.brute(a, b, **kw)), (name, h, w, kw)
                    n += 1
    assert n > 300


def test_reference_equals_bincount():
    for h, w in ((33, 63), (40, 130)):
        for name, a, b in pairs_of(h, w):
            r = CR.compare(a, b, rows_a=6, rows_b=5)
            ok = (a < 6) & (b < 5)
            flat = np.bincount(a[ok].astype(np.int64) * 5 + b[ok], minlength=30).reshape(6, 5)
            assert (r.matrix == flat).all(), name
            assert (r.a[:, CR.PIXELS] == np.bincount(a[ok], minlength=6)).all() and (r.b[:, CR.PIXELS] == np.bincount(b[ok], minlength=5)).all()


def test_identities():
    for h, w in SMALL:
        for name, a, b in pairs_of(h, w):
            for kw in settings():
                r = CR.compare(a, b, **kw)
                c = r.counts
                inside = int(c[CR.COMPARED]) - int(c[CR.OUTSIDE])
                assert int(c[CR.COMPARED]) + int(c[CR.IGNORED]) == h * w
                assert int(r.matrix.sum()) == inside == int(r.a[:, CR.PIXELS].sum()) == int(r.b[:, CR.PIXELS].sum())
                assert (r.matrix.sum(axis=1) == r.a[:, CR.PIXELS]).all() and (r.matrix.sum(axis=0) == r.b[:, CR.PIXELS]).all()
                assert int(np.trace(r.matrix[:min(r.matrix.shape), :min(r.matrix.shape)])) == c[CR.EQUAL]
                assert c[CR.PAIRS] == (r.matrix != 0).sum() <= c[CR.RUNS] <= max(inside, 0)
                assert c[CR.MATCHED] == CR.matched(r.a).sum() == CR.matched(r.b).sum()


def test_swapping_the_planes_transposes():
    for h, w in SMALL:
        for name, a, b in pairs_of(h, w):
            x = CR.compare(a, b, flags=CR.IGNORE_A, ignore_a=1, rows_a=4, rows_b=5)
            y = CR.compare(b, a, flags=CR.IGNORE_B, ignore_b=1, rows_a=5, rows_b=4)
            assert (x.matrix.T == y.matrix).all() and (x.a == y.b).all() and (x.b == y.a).all() and (x.counts == y.counts).all()


def test_a_plane_against_itself():
    for h, w in SMALL:
        k = R.noise(h, w, 5, seed=h)
        r = CR.compare(k, k, rows_a=6, rows_b=6)
        assert (r.matrix == np.diag(np.bincount(k.ravel(), minlength=6))).all() and (r.a == r.b).all()
        present = r.a[:, CR.PIXELS] > 0
        assert (CR.matched(r.a) == present).all() and (r.a[present, CR.INTER] == r.a[present, CR.UNION]).all()
        assert (r.a[present, CR.PARTNER] == np.flatnonzero(present)).all() and r.counts[CR.MATCHED] == present.sum() == r.counts[CR.PAIRS]
        assert r.counts[CR.EQUAL] == h * w


def test_matched_implies_mutual_best_partner():
    seen = 0
    for seed in range(12):
        a = R.smooth(40, 70, seed=seed, classes=6, cell=8)
        b = CR.shifted(a, 1 + seed % 3, seed % 4 + 1) if seed & 1 else R.smooth(40, 70, seed=seed + 100, classes=6, cell=8)
        la, lb = R.label(a)[0], R.label(b)[0]
        n_a, n_b = int(la.max()) + 1, int(lb.max()) + 1
        r = CR.compare(la, lb, rows_a=n_a, rows_b=n_b)
        for i in np.flatnonzero(CR.matched(r.a)):
            j = int(r.a[i, CR.PARTNER])
            assert r.b[j, CR.PARTNER] == i and r.b[j, CR.INTER] == r.a[i, CR.INTER] and r.b[j, CR.UNION] == r.a[i, CR.UNION]
            assert CR.matched(r.b)[j]
            seen += 1
    assert seen > 20


def test_overflow_rule_of_the_reference():
    a, b = R.noise(33, 63, 3, seed=1), R.noise(33, 63, 3, seed=2)
    full = CR.compare(a, b, rows_a=64, rows_b=65)
    assert full.counts[CR.STATUS] == CR.TABLE and 2 * int(full.counts[CR.RUNS]) > 64
    o = CR.compare(a, b, rows_a=64, rows_b=65, pair_slots=64)
    assert o.counts[CR.STATUS] == CR.TABLE | CR.OVERFLOW and o.counts[CR.PAIRS] == 0 == o.counts[CR.MATCHED]
    assert (o.matrix == full.matrix).all() and (o.a[:, CR.PIXELS] == full.a[:, CR.PIXELS]).all() and (o.counts[:4] == full.counts[:4]).all()
    assert (o.a[:, 1:] == [NONE, 0, 0]).all() and (o.b[:, 1:] == [NONE, 0, 0]).all()
    assert CR.compare(a, b, rows_a=64, rows_b=64, pair_slots=64).counts[CR.STATUS] == 0  # the dense form cannot overflow
    # 2 R == pair_slots exactly: no overflow
    exact = np.zeros((1, 64), np.uint8)
    exact[0, :31] = np.arange(31) % 2
    exact[0, 31:] = 2  # 31 + 1 = 32 runs: 2 R == 64
    r = CR.compare(exact, exact, rows_a=64, rows_b=65, pair_slots=64)
    assert r.counts[CR.RUNS] == 32 and r.counts[CR.STATUS] == CR.TABLE and r.counts[CR.PAIRS] == 3


def test_confusion_summary_on_hand_worked_cases():
    s = confusion_summary([[5, 1], [2, 2]], names=["sky", "sea"])
    assert s["pixel_accuracy"] == 7 / 10
    assert [(c["name"], c["intersection"], c["union"]) for c in s["classes"]] == [("sky", 5, 8), ("sea", 2, 5)]
    assert s["miou"] == pytest.approx((5 / 8 + 2 / 5) / 2) and s["fwiou"] == pytest.approx((7 * 5 / 8 + 3 * 2 / 5) / 10)
    # a class neither plane holds has no IoU and does not enter the mean
    s = confusion_summary([[4, 0, 0], [0, 0, 0], [1, 0, 3]])
    assert [c["iou"] for c in s["classes"]] == [4 / 5, None, 3 / 4] and s["miou"] == pytest.approx((0.8 + 0.75) / 2)
    assert s["classes"][0]["name"] == "__background__"  # the library's names by default
    k = R.noise(9, 11, 4)
    s = confusion_summary(CR.compare(k, k, rows_a=4, rows_b=4).matrix)
    assert s["pixel_accuracy"] == 1.0 == s["miou"] == s["fwiou"]
    e = confusion_summary(np.zeros((3, 3), np.uint32))
    assert e["pixel_accuracy"] is None and e["miou"] is None and e["fwiou"] is None
    assert confusion_summary(np.array([[1, 2, 3]], np.uint32))["classes"][0]["union"] == 6  # not square: padded with zeros


def test_panoptic_summary_on_hand_worked_cases():
    # a: segments 0 (class 1, 10 px), 1 (class 1, 6 px), 2 (class 2, 4 px);  b: 0 (class 1, 9 px), 1 (class 2, 8 px), 2 (class 1, 3 px)
    rows_a = [[10, 0, 8, 11], [6, 1, 4, 10], [4, 1, 4, 8]]
    rows_b = [[9, 0, 8, 11], [8, 1, 4, 10], [3, 0, 2, 11]]
    p = panoptic_summary(rows_a, rows_b, [1, 1, 2], [1, 2, 1])
    # (0, 0) matches, IoU 8/11, class 1.  a's 1 is unmatched (4/10): FP of class 1.  a's 2 has IoU 4/8, not above one half: FP of class 2.
    # b's 1 (class 2) and 2 (class 1) are FN.
    assert p["classes"][1] == {"tp": 1, "fp": 1, "fn": 1, "sum_iou": 8 / 11, "pq": (8 / 11) / 2, "sq": 8 / 11, "rq": 0.5}
    assert p["classes"][2] == {"tp": 0, "fp": 1, "fn": 1, "sum_iou": 0.0, "pq": 0.0, "sq": 0.0, "rq": 0.0}
    assert p["pq"] == pytest.approx(2 / 11) and p["rq"] == 0.25
    # a matched pair whose classes differ is a false positive and a false negative
    q = panoptic_summary([[5, 0, 5, 5]], [[5, 0, 5, 5]], [1], [2])
    assert q["classes"] == {1: {"tp": 0, "fp": 1, "fn": 0, "sum_iou": 0.0, "pq": 0.0, "sq": 0.0, "rq": 0.0},
                            2: {"tp": 0, "fp": 0, "fn": 1, "sum_iou": 0.0, "pq": 0.0, "sq": 0.0, "rq": 0.0}}
    # identical label planes: PQ = SQ = RQ = 1, with the classes from Regions' table
    k = R.smooth(40, 70, seed=3, classes=5, cell=8)
    labels, table, n = R.label(k)
    r = CR.compare(labels, labels, rows_a=n + 2, rows_b=n + 2)
    klass = list(table[:, _lib.REGION_CLASS]) + [0, 0]
    p = panoptic_summary(r.a, r.b, klass, klass)
    assert p["pq"] == p["sq"] == p["rq"] == 1.0 and sum(c["tp"] for c in p["classes"].values()) == n
    assert panoptic_summary(np.zeros((0, 4)), np.zeros((0, 4)), [], [])["pq"] is None


def test_cli_argument_errors():
    import io
    from contextlib import redirect_stderr

    from infur_amd import segments_cli

    base = ["--width", "8", "--height", "8", "--synthetic-weights"]
    for extra, word in ((["--truth-ignore", "255"], "--truth-ignore needs --truth"), (["--truth", "t.u8", "--truth-ignore", "256"], "a byte"),
                        (["--truth", "t.u8", "--truth-ignore", "-1"], "a byte")):
        err = io.StringIO()
        with redirect_stderr(err), pytest.raises(SystemExit) as e:
            segments_cli.main(base + extra)
        assert e.value.code == 2 and word in err.getvalue(), extra
