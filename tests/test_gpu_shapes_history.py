"""What Shapes writes must not depend on what its context ran before (the idea of tests/test_gpu_history.py and
tests/test_gpu_stage_history.py, for the stage that came after them).

The stage's scratch only grows and is never cleared as a whole: a call lays its scan sums, ranks, hull ids, signs and keep flags
into it at offsets computed from its rows and clears exactly what it believes it needs.  A small TARGET call runs in a context that
has run nothing else, in one that ran larger and denser calls of the same stage first (more loops, longer loops, hulls of more
than one stride, truncated and malformed input that stops half-way), and in one the other decode stages have used.  Every
comparison is of bytes, and of both against the numpy reference -- "all equal" must not be able to mean "all equally wrong"."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import outlines_ref as O  # noqa: E402
import regions_ref as R  # noqa: E402
import shapes_ref as H  # noqa: E402
import simplify_ref as S  # noqa: E402
from test_gpu_anchors import dev_anchors  # noqa: E402
from test_gpu_outlines import dev_outlines  # noqa: E402
from test_gpu_regions import dev_regions  # noqa: E402
from test_gpu_runs import dev_runs  # noqa: E402
from test_gpu_shapes import OUTPUTS, dev_shapes  # noqa: E402
from test_gpu_sieve import dev_sieve  # noqa: E402
from test_gpu_simplify import dev_simplify  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd.processors import Context  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = R.smooth(13, 70, seed=5, classes=5, cell=4)
TARGET_LOOPS = O.outline(TARGET, O.CONN8)
TARGET_SKIP = O.outline(TARGET, O.SKIP, 0)
ROWS = 7


def target_calls(ctx):
    """-> the bytes of every output of the small calls"""
    out = {}
    for tag, (l, v, c), kw in (("all ", TARGET_LOOPS, {}), ("skip ", TARGET_SKIP, {}), ("short ", TARGET_LOOPS, dict(loops_rows_out=3, vertex_rows_out=5, shape_rows=2)),
                               ("cut ", TARGET_LOOPS, dict(loops_rows_in=len(TARGET_LOOPS[0]) - 1))):
        got = dev_shapes(ctx, l, v, c, 13, 70, rows=ROWS, **kw)
        out.update({tag + name: got[name].tobytes() for name in OUTPUTS})
    return out


def reference():
    out = {}
    for tag, (l, v, c) in (("all ", TARGET_LOOPS), ("skip ", TARGET_SKIP)):
        r = H.shapes(l, v, c, 70, rows=ROWS)
        out.update({tag + name: a.tobytes() for name, a in zip(OUTPUTS, r)})
    return out


@pytest.fixture(scope="module")
def fresh():
    assert _lib.load().infur_features() & _lib.FEATURE_SHAPES  # (fails on a library without the feature)
    with Context(device=0) as c:
        got = target_calls(c)
    for name, want in reference().items():  # the buffers are longer than what is written: the reference is their head
        assert got[name][:len(want)] == want, name
    return got


def test_after_larger_and_denser_calls_of_the_same_stage(fresh):
    noise = R.noise(65, 129, 5, seed=4)
    nl, nv, nc = O.outline(noise)
    disc = H.disc(120)
    comb = S.comb(40, 700)
    with Context(device=0) as c:
        dev_shapes(c, nl, nv, nc, 65, 129, rows=40)  # more loops, more rows
        dev_shapes(c, *O.outline(disc, O.SKIP, 0), 243, 243, rows=2)  # a hull of more than one stride
        dev_shapes(c, *O.outline(comb, O.SKIP, 0), 40, 700, rows=2, vertex_rows_in=70000)  # one long loop, many more rows than vertices
        dev_shapes(c, nl, nv, nc, 65, 129, rows=3, vertex_rows_in=len(nv) - 1)  # truncated: the launches see nothing
        bad = nl.copy()
        bad[1::2, 1] = 1
        dev_shapes(c, bad, nv, nc, 65, 129, rows=9)  # every second record malformed
        got = target_calls(c)
    assert got.keys() == fresh.keys()
    for name in fresh:
        assert got[name] == fresh[name], name


def test_after_the_other_decode_stages(fresh):
    noise = R.noise(40, 130, 7, seed=2)
    labels, _, n = R.label(noise, connectivity=R.CONNECT_8)
    ol, ov, oc = O.outline(noise)
    with Context(device=0) as c:
        dev_regions(c, noise, None, R.CONNECT_8, table_rows=n)
        dev_runs(c, labels, 0, 0, rows=40 * 130)
        dev_outlines(c, noise, 0, 0, 0, 40 * 130, 4 * 40 * 130)
        dev_simplify(c, ol, ov, oc, 40, 130, 16)
        dev_anchors(c, labels, 0, 0, rows=n)
        dev_sieve(c, noise, R.CONNECT_4, 8, max_rounds=4)
        got = target_calls(c)
        dev_simplify(c, ol, ov, oc, 40, 130, 16)  # and they still work behind it
        assert np.frombuffer(got["all counts"], np.uint32)[0] == TARGET_LOOPS[2][0]
    for name in fresh:
        assert got[name] == fresh[name], name
