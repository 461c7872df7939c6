"""Adjacency and Sieve (the region adjacency graph, and speckle regions merged into their neighbours) without a GPU: the ABI
surface, the reference the GPU tests use (tests/sieve_ref.py) against plain double loops, the header's worked example word for
word, the reference's own identities, the invariant the stage exists for, the facts of a prototype, and the host helpers."""
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib
from infur_amd.processors import adjacency_graph, sieve_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import sieve_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_adjacency", "infur_adjacency_dev", "infur_sieve", "infur_sieve_dev", "infur_frame_sieve", "infur_frame_sieve_dev")
CONSTANTS = {"INFUR_ADJ_SKIP": 1, "INFUR_ADJ_A": 0, "INFUR_ADJ_B": 1, "INFUR_ADJ_BORDER": 2, "INFUR_ADJ_FIRST": 3, "INFUR_ADJ_PAIR_WORDS": 4,
             "INFUR_ADJ_DEGREE": 0, "INFUR_ADJ_LONGEST": 1, "INFUR_ADJ_ROW_BORDER": 2, "INFUR_ADJ_PERIMETER": 3, "INFUR_ADJ_ROW_WORDS": 4,
             "INFUR_ADJ_PAIRS": 0, "INFUR_ADJ_EDGES": 1, "INFUR_ADJ_SKIPPED": 2, "INFUR_ADJ_OUTSIDE": 3, "INFUR_ADJ_RUNS": 4, "INFUR_ADJ_WRITTEN": 5,
             "INFUR_ADJ_STATUS": 7, "INFUR_ADJ_COUNT_WORDS": 8, "INFUR_ADJ_OVERFLOW": 1, "INFUR_ADJ_TRUNCATED": 2,
             "INFUR_SIEVE_CLASS": 0, "INFUR_SIEVE_INTO": 1, "INFUR_SIEVE_ROUND": 2, "INFUR_SIEVE_BORDER": 3, "INFUR_SIEVE_ROW_WORDS": 4,
             "INFUR_SIEVE_REGIONS": 0, "INFUR_SIEVE_SMALL": 1, "INFUR_SIEVE_ABSORBED": 2, "INFUR_SIEVE_STRANDED": 3, "INFUR_SIEVE_ROUNDS": 4,
             "INFUR_SIEVE_PIXELS_CHANGED": 5, "INFUR_SIEVE_PAIRS": 6, "INFUR_SIEVE_STATUS": 7, "INFUR_SIEVE_COUNT_WORDS": 8,
             "INFUR_SIEVE_OVERFLOW": 1, "INFUR_SIEVE_ROUNDS_EXHAUSTED": 2, "INFUR_SIEVE_TABLE_SHORT": 4, "INFUR_FEATURE_SIEVE": 1024}
NONE = S.NONE
SMALL = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (2, 130), (13, 70))
MIN_PIXELS = (0, 1, 2, 8, 64)


def planes_of(h, w):
    yield "smooth", R.smooth(h, w, seed=h + w, classes=5, cell=4)
    yield "noise", R.noise(h, w, 4, seed=w)
    yield "single", R.single(h, w)
    yield "stripes", R.stripes(h, w)
    yield "checkerboard", R.checkerboard(h, w)


def same_adj(x, y):
    return x.pairs.shape == y.pairs.shape and (x.pairs == y.pairs).all() and (x.rows == y.rows).all() and (x.counts == y.counts).all()


def same_sieve(x, y):
    return (x.klass_out == y.klass_out).all() and x.rows.shape == y.rows.shape and (x.rows == y.rows).all() and (x.counts == y.counts).all()


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_SIEVE
    assert _lib.FEATURE_SIEVE == 1024 and lib.infur_features() & 1023 == 1023  # the ten older bits stay set
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
    for name in ("INFUR_ADJ_NONE", "INFUR_SIEVE_NONE"):
        assert "#define %s 0xFFFFFFFFu" % name in header and getattr(_lib, name[len("INFUR_"):]) == NONE
        assert "pub const %s: u32 = 0xFFFF_FFFF;" % name in rust
    assert (S.SKIP, S.PAIR_WORDS, S.ROW_WORDS, S.COUNT_WORDS, S.OVERFLOW, S.TRUNCATED) == (1, 4, 4, 8, 1, 2)
    assert (S.A, S.B, S.BORDER, S.FIRST) == (_lib.ADJ_A, _lib.ADJ_B, _lib.ADJ_BORDER, _lib.ADJ_FIRST)
    assert (S.DEGREE, S.LONGEST, S.ROW_BORDER, S.PERIMETER) == (_lib.ADJ_DEGREE, _lib.ADJ_LONGEST, _lib.ADJ_ROW_BORDER, _lib.ADJ_PERIMETER)
    assert [S.PAIRS, S.EDGES, S.SKIPPED, S.OUTSIDE, S.RUNS, S.WRITTEN, S.RESERVED, S.STATUS] == list(range(8))
    assert (S.S_CLASS, S.S_INTO, S.S_ROUND, S.S_BORDER, S.SIEVE_ROW_WORDS) == (0, 1, 2, 3, 4)
    assert [S.S_REGIONS, S.S_SMALL, S.S_ABSORBED, S.S_STRANDED, S.S_ROUNDS, S.S_PIXELS_CHANGED, S.S_PAIRS, S.S_STATUS] == list(range(8))
    assert (S.S_OVERFLOW, S.S_ROUNDS_EXHAUSTED, S.S_TABLE_SHORT, S.DEFAULT_ROUNDS, S.MAX_ROUNDS, S.DEFAULT_SLOTS) == (1, 2, 4, 8, 64, 1 << 20)


def test_rejected_calls_need_no_gpu(lib):
    """a NULL context, and with it a bad pair_slots, max_rounds = 65 and elem = 2: refused, and no output touched"""
    b = np.full(64, 0x5A5A5A5A, np.uint32)
    p = b.ctypes.data
    ow, oh = _lib.C.c_uint32(0), _lib.C.c_uint32(0)
    for elem, slots in ((1, 0), (2, 0), (1, 48), (1, 32)):
        assert lib.infur_adjacency(None, p, elem, 2, 2, 0, 0, 4, p, 4, p, p, slots) == _lib.E_INVALID_ARG
        assert lib.infur_adjacency_dev(None, p, elem, 2, 2, 0, 0, 4, p, 4, p, p, slots) == _lib.E_INVALID_ARG
    for rounds, slots in ((0, 0), (65, 0), (8, 100)):
        assert lib.infur_sieve(None, p, p, p, 1, 1, 2, 2, 2, rounds, slots, p, p, p) == _lib.E_INVALID_ARG
        assert lib.infur_sieve_dev(None, p, p, p, 1, p, 2, 2, 2, rounds, slots, p, p, p) == _lib.E_INVALID_ARG
        for f in (lib.infur_frame_sieve, lib.infur_frame_sieve_dev):
            assert f(None, p, 2, 2, 1.0, 0, 0, 8, 2, 0, p, p, 4, p, 16, p, 1, p, p, ow, oh, rounds, slots, p, p) == _lib.E_INVALID_ARG
    assert (b == 0x5A5A5A5A).all() and ow.value == 0 == oh.value


def test_the_worked_example_word_for_word():
    labels, table, n = R.label(S.WORKED, connectivity=R.CONNECT_4)
    assert labels.tolist() == [[0, 0, 0, 1, 1, 1], [0, 2, 0, 1, 1, 1], [0, 0, 0, 1, 3, 3], [0, 0, 0, 1, 3, 4]]
    assert (labels == R.label(S.WORKED, connectivity=R.CONNECT_8)[0]).all()
    assert table[:, [R.PIXELS, R.CLASS]].tolist() == [[11, 1], [8, 2], [1, 3], [3, 4], [1, 5]]
    a = S.adjacency(labels, 5)
    assert a.pairs.tolist() == [[0, 2, 4, 3], [0, 1, 4, 4], [1, 3, 4, 21], [3, 4, 2, 35]]
    assert a.rows.tolist() == [[2, 1, 4, 18], [2, 0, 4, 14], [1, 0, 4, 4], [2, 1, 4, 8], [1, 3, 2, 4]]
    assert a.counts.tolist() == [4, 14, 0, 0, 9, 4, 0, 0]  # PAIRS EDGES SKIPPED OUTSIDE RUNS WRITTEN 0 STATUS
    assert same_adj(a, S.brute_adjacency(labels, 5))
    s = S.sieve(S.WORKED, labels, table, n, min_pixels=4)
    assert s.rows.tolist() == [[1, 0, 0, 0], [2, 1, 0, 0], [1, 0, 1, 4], [2, 1, 1, 4], [2, 1, 2, 2]]
    assert s.klass_out.tolist() == [[1, 1, 1, 2, 2, 2]] * 4
    assert s.counts.tolist() == [5, 3, 3, 0, 2, 5, 4, 0]  # REGIONS SMALL ABSORBED STRANDED ROUNDS PIXELS_CHANGED PAIRS STATUS
    assert same_sieve(s, S.brute_sieve(S.WORKED, labels, table, n, min_pixels=4))
    assert sieve_summary(s.counts) == {"regions": 5, "small": 3, "absorbed": 3, "stranded": 0, "rounds": 2, "pixels_changed": 5, "pairs": 4,
                                       "status": 0, "overflow": False, "rounds_exhausted": False, "table_short": False}
    g = adjacency_graph(a.pairs, 5)
    assert g == {0: [(1, 4), (2, 4)], 1: [(0, 4), (3, 4)], 2: [(0, 4)], 3: [(1, 4), (4, 2)], 4: [(3, 2)]}
    assert all(g[v][0][0] == a.rows[v, S.LONGEST] for v in g)
    # one round is not enough for region 4, and says so
    one = S.sieve(S.WORKED, labels, table, n, min_pixels=4, max_rounds=1)
    assert one.counts.tolist() == [5, 3, 2, 1, 1, 4, 4, S.S_ROUNDS_EXHAUSTED] and one.rows[4].tolist() == [5, 4, NONE, 0]


def adjacency_settings(k):
    """class plane settings, then the label planes of both connectivities"""
    top = int(k.max())
    yield k, dict(rows=top + 1)
    yield k, dict(rows=max(top, 1))  # the largest value is outside
    yield k, dict(rows=top + 2, flags=S.SKIP, skip_value=0)
    yield k, dict(rows=top + 1, flags=S.SKIP, skip_value=1, pair_rows=2)
    for conn in (R.CONNECT_4, R.CONNECT_8):
        labels, _, n = R.label(k, connectivity=conn)
        yield labels, dict(rows=n)
        yield labels, dict(rows=max(n - 1, 0), pair_slots=64)
        filtered = R.label(k, connectivity=conn, min_pixels=3)
        yield filtered[0], dict(rows=filtered[2] + 1, flags=S.SKIP, skip_value=NONE)


def test_adjacency_reference_equals_the_brute_force_loops():
    cases = 0
    for h, w in SMALL:
        for name, k in planes_of(h, w):
            for plane, kw in adjacency_settings(k):
                assert same_adj(S.adjacency(plane, **kw), S.brute_adjacency(plane, **kw)), (name, h, w, kw)
                cases += 1
    assert cases > 300


def test_sieve_reference_equals_the_brute_force_loops():
    cases = 0
    for h, w in SMALL:
        for name, k in planes_of(h, w):
            for conn in (R.CONNECT_4, R.CONNECT_8):
                labels, table, n = R.label(k, connectivity=conn)
                for mp in MIN_PIXELS:
                    kw = dict(min_pixels=mp, max_rounds=3 if mp == 8 else 0)
                    assert same_sieve(S.sieve(k, labels, table, n, **kw), S.brute_sieve(k, labels, table, n, **kw)), (name, h, w, conn, mp)
                    cases += 1
                # a short table: the regions beyond it are fixed
                kw = dict(table_rows=n // 2, min_pixels=8)
                assert same_sieve(S.sieve(k, labels, table, n, **kw), S.brute_sieve(k, labels, table, n, **kw)), (name, h, w, conn)
                cases += 1
    assert cases > 300


def test_identities():
    for h, w in SMALL:
        for name, k in planes_of(h, w):
            for plane, kw in adjacency_settings(k):
                a = S.adjacency(plane, **dict(kw, pair_rows=None))
                c = a.counts
                assert int(a.pairs[:, S.BORDER].sum()) == c[S.EDGES]
                assert int(a.rows[:, S.DEGREE].sum()) == 2 * int(c[S.PAIRS])
                assert c[S.PAIRS] <= c[S.RUNS] and (c[S.STATUS] & S.OVERFLOW or c[S.RUNS] <= c[S.EDGES])
                assert (np.diff(a.pairs[:, S.FIRST].astype(np.int64)) > 0).all() and (a.pairs[:, S.A] < a.pairs[:, S.B]).all()
                assert c[S.WRITTEN] == c[S.PAIRS] == len(a.pairs)
    labels, _, n = R.label(R.stripes(5, 64), connectivity=R.CONNECT_4)
    a = S.adjacency(labels, n)
    assert n == 64 and a.counts[S.RUNS] == 63 == a.counts[S.PAIRS] and (a.pairs[:, S.BORDER] == 5).all()
    # 2 R == pair_slots exactly: no overflow
    alt = (np.arange(33) % 2).astype(np.uint8)[None]
    a = S.adjacency(alt, 2, pair_slots=64)
    assert a.counts[S.RUNS] == 32 and a.counts[S.STATUS] == 0 and a.counts[S.PAIRS] == 1 and a.pairs.tolist() == [[0, 1, 32, 0]]
    alt = (np.arange(34) % 2).astype(np.uint8)[None]
    o = S.adjacency(alt, 2, pair_slots=64)
    assert o.counts.tolist() == [0, 0, 0, 0, 33, 0, 0, S.OVERFLOW] and o.rows.tolist() == [[0, NONE, 0, 68], [0, NONE, 0, 68]]
    # truncation is reported only where records are wanted
    k = R.noise(7, 65, 4, seed=2)
    assert S.adjacency(k, 4, pair_rows=2).counts[S.STATUS] == S.TRUNCATED and len(S.adjacency(k, 4, pair_rows=2).pairs) == 2
    assert S.adjacency(k, 4, pair_rows=0, want_pairs=False).counts[[S.WRITTEN, S.STATUS]].tolist() == [0, 0]


def test_the_invariant_the_stage_exists_for():
    seen = 0
    for h, w in SMALL + ((33, 63), (40, 130)):
        for name, k in planes_of(h, w):
            for conn in (R.CONNECT_4, R.CONNECT_8):
                labels, table, n = R.label(k, connectivity=conn)
                for mp in MIN_PIXELS:
                    s = S.sieve(k, labels, table, n, min_pixels=mp, max_rounds=64)
                    kept = table[:, R.PIXELS] >= mp
                    assert (s.klass_out[kept[labels]] == k[kept[labels]]).all(), (name, h, w)  # the pixels of kept regions are unchanged
                    assert s.counts[S.S_SMALL] == (~kept).sum() and s.counts[S.S_ABSORBED] + s.counts[S.S_STRANDED] == s.counts[S.S_SMALL]
                    if s.counts[S.S_STRANDED] == 0:
                        for c2 in (conn, R.CONNECT_8):  # (the labelling's own connectivity, and the coarser one)
                            assert int(R.label(s.klass_out, connectivity=c2)[1][:, R.PIXELS].min()) >= mp, (name, h, w, conn, mp, c2)
                        seen += 1
                    else:  # stranded regions have no kept region to reach: everything is small
                        assert not kept.any() or s.counts[S.S_STATUS] & S.S_ROUNDS_EXHAUSTED
    assert seen > 200


def test_facts_of_the_prototype():
    k = R.smooth(40, 70, seed=3, classes=6, cell=8)
    s, labels, table, n = S.sieve_plane(k, R.CONNECT_8, 64)
    assert s.counts.tolist() == [48, 33, 33, 0, 2, 664, 103, 0] and S.adjacency(labels, n).counts[S.RUNS] == 486
    cleaned = R.label(s.klass_out, connectivity=R.CONNECT_8)
    assert cleaned[2] == 14 and int(cleaned[1][:, R.PIXELS].min()) == 78 and int((s.klass_out != k).sum()) == 664
    k = R.noise(65, 129, 5, seed=4)
    s, labels, table, n = S.sieve_plane(k, R.CONNECT_4, 8, max_rounds=64)
    assert s.counts[:5].tolist() == [5193, 5162, 5162, 0, 17] and s.counts[S.S_STATUS] == 0
    s = S.sieve(k, labels, table, n, min_pixels=8)
    assert s.counts[S.S_ROUNDS] == 8 and s.counts[S.S_STATUS] == S.S_ROUNDS_EXHAUSTED and s.counts[S.S_STRANDED] > 0
    assert S.sieve(k, labels, table, n, min_pixels=8, max_rounds=17).counts[[S.S_STRANDED, S.S_STATUS]].tolist() == [0, 0]
    k = R.noise(33, 63, 3, seed=1)
    s, labels, table, n = S.sieve_plane(k, R.CONNECT_4, 64)
    assert s.counts[:6].tolist() == [767, 767, 0, 767, 0, 0] and (s.klass_out == k).all() and (s.rows[:, S.S_ROUND] == NONE).all()
    k = R.single(9, 11)
    s, labels, table, n = S.sieve_plane(k, R.CONNECT_8, 64)
    assert s.counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and (s.klass_out == k).all() and s.rows.tolist() == [[3, 0, 0, 0]]
    # overflow: the plane is copied and every small region is stranded
    k = R.smooth(40, 70, seed=3, classes=6, cell=8)
    s, labels, table, n = S.sieve_plane(k, R.CONNECT_8, 64, pair_slots=64)
    assert s.counts.tolist() == [48, 33, 0, 33, 0, 0, 0, S.S_OVERFLOW] and (s.klass_out == k).all()


def test_cli_argument_errors():
    import io
    from contextlib import redirect_stderr

    from infur_amd import segments_cli

    base = ["--width", "8", "--height", "8", "--synthetic-weights"]
    for extra, word in ((["--sieve-rounds", "4"], "--sieve-rounds needs --sieve"), (["--sieve", "0"], "at least 1"),
                        (["--sieve", "8", "--sieve-rounds", "65"], "1 to 64"), (["--sieve", "8", "--sieve-rounds", "0"], "1 to 64"),
                        (["--sieve", "8", "--tracks"], "--sieve does not combine"), (["--sieve", "8", "--truth", "t.u8"], "--sieve does not combine"),
                        (["--sieve", "8", "--runs-out", "r.bin"], "--sieve does not combine")):
        err = io.StringIO()
        with redirect_stderr(err), pytest.raises(SystemExit) as e:
            segments_cli.main(base + extra)
        assert e.value.code == 2 and word in err.getvalue(), extra
