"""What Adjacency and Sieve write must not depend on what their context ran before (the idea of tests/test_gpu_history.py and
tests/test_gpu_stage_history.py, for the stage that came after them).

The stage's scratch only grows and is never cleared as a whole: a call lays its accumulators, pair table, bitmap and per-region
state into it at offsets computed from its arguments and clears exactly what it believes it needs.  A small TARGET call runs in a
context that has run nothing else, in one that ran larger and denser calls of the same stage first (more slots, more rows, more
rounds, an overflow that stops half-way), and in one the other decode stages have used.  Every comparison is of bytes, and of
both against the numpy reference -- "all equal" must not be able to mean "all equally wrong"."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import regions_ref as R  # noqa: E402
import sieve_ref as S  # noqa: E402
from test_gpu_anchors import dev_anchors  # noqa: E402
from test_gpu_compare import dev_compare  # noqa: E402
from test_gpu_outlines import dev_outlines  # noqa: E402
from test_gpu_regions import dev_regions  # noqa: E402
from test_gpu_runs import dev_runs  # noqa: E402
from test_gpu_sieve import ADJ_OUTPUTS, SIEVE_OUTPUTS, dev_adjacency, dev_sieve  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd.processors import Context  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = R.smooth(13, 70, seed=5, classes=5, cell=4)
TARGET_LABELS, TARGET_TABLE, TARGET_N = R.label(TARGET, connectivity=R.CONNECT_8)


def target_calls(ctx):
    """-> the bytes of every output of the small calls"""
    out = {}
    a = dev_adjacency(ctx, TARGET_LABELS, TARGET_N, pair_rows=256, pair_slots=1024)
    out.update({"adj " + name: a[name].tobytes() for name in ADJ_OUTPUTS})
    a = dev_adjacency(ctx, TARGET, 6, flags=S.SKIP, skip_value=0, pair_rows=32, pair_slots=64 * 1024)
    out.update({"adj klass " + name: a[name].tobytes() for name in ADJ_OUTPUTS})
    for mp, slots in ((8, 1024), (64, 0)):
        s = dev_sieve(ctx, TARGET, R.CONNECT_8, mp, max_rounds=4, pair_slots=slots)
        out.update({f"sieve {mp} " + name: s[name].tobytes() for name in SIEVE_OUTPUTS})
    return out


def reference():
    out = {}
    a = S.adjacency(TARGET_LABELS, TARGET_N, pair_rows=256, pair_slots=1024)
    b = S.adjacency(TARGET, 6, flags=S.SKIP, skip_value=0, pair_rows=32, pair_slots=64 * 1024)
    for tag, r in (("adj ", a), ("adj klass ", b)):
        out[tag + "rows"], out[tag + "counts"], out[tag + "pairs"] = r.rows.tobytes(), r.counts.tobytes(), r.pairs.tobytes()
    for mp, slots in ((8, 1024), (64, 0)):
        s = S.sieve(TARGET, TARGET_LABELS, TARGET_TABLE, TARGET_N, min_pixels=mp, max_rounds=4, pair_slots=slots)
        out[f"sieve {mp} klass_out"], out[f"sieve {mp} counts"], out[f"sieve {mp} rows"] = s.klass_out.tobytes(), s.counts.tobytes(), s.rows.tobytes()
    return out


@pytest.fixture(scope="module")
def fresh():
    assert _lib.load().infur_features() & _lib.FEATURE_SIEVE  # (fails on a library without the feature)
    with Context(device=0) as c:
        got = target_calls(c)
    ref = reference()
    for name, want in ref.items():  # pair and row buffers are longer than what is written: the reference is their head
        assert got[name][:len(want)] == want, name
    return got


def test_after_larger_and_denser_calls_of_the_same_stage(fresh):
    noise = R.noise(65, 129, 5, seed=4)
    labels, _, n = R.label(noise, connectivity=R.CONNECT_4)
    with Context(device=0) as c:
        dev_adjacency(c, labels, n, pair_rows=16384)  # more rows, the default 2^20 slots, a longer bitmap
        dev_adjacency(c, noise, 5, pair_rows=64, pair_slots=64)  # an overflow: the table stays as the memset left it
        dev_sieve(c, noise, R.CONNECT_4, 8, max_rounds=64)  # more regions, more rounds
        dev_sieve(c, noise, R.CONNECT_4, 8, max_rounds=2, pair_slots=4096)  # stops with regions unresolved, or overflows
        dev_sieve(c, R.checkerboard(40, 130), R.CONNECT_4, 2)  # every region small: nothing resolves
        got = target_calls(c)
    assert got.keys() == fresh.keys()
    for name in fresh:
        assert got[name] == fresh[name], name


def test_after_the_other_decode_stages(fresh):
    noise = R.noise(40, 130, 7, seed=2)
    labels, _, n = R.label(noise, connectivity=R.CONNECT_8)
    with Context(device=0) as c:
        dev_regions(c, noise, None, R.CONNECT_8, table_rows=n)
        dev_compare(c, labels, labels[::-1].copy(), rows_a=n, rows_b=n, pair_slots=1 << 16, want=("a", "b", "counts"))  # the table form
        dev_runs(c, labels, 0, 0, rows=40 * 130)
        dev_outlines(c, noise, 0, 0, 0, 40 * 130, 4 * 40 * 130)
        dev_anchors(c, labels, 0, 0, rows=n)
        got = target_calls(c)
        dev_regions(c, noise, None, R.CONNECT_4, table_rows=n)  # and they still work behind it
    for name in fresh:
        assert got[name] == fresh[name], name
