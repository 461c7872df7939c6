"""What Raster writes must not depend on what its context ran before (the idea of tests/test_gpu_history.py and
tests/test_gpu_stage_history.py, for the stage that came after them).

The stage's accumulator only grows and is never cleared as a whole: a call clears the head words and one 64-bit word per pixel of
ITS plane and adds its crossings to them.  A small TARGET call runs in a context that has run nothing else, in one that ran larger
and denser calls of the same stage first (a larger plane, every pixel side a crossing, conflicts that leave words far from zero,
truncated input that clears and then stops), and in one the other decode stages have used.  Every comparison is of bytes, and of
both against the numpy reference -- "all equal" must not be able to mean "all equally wrong"."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import outlines_ref as O  # noqa: E402
import raster_ref as A  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as RR  # noqa: E402
from test_gpu_anchors import dev_anchors  # noqa: E402
from test_gpu_outlines import dev_outlines  # noqa: E402
from test_gpu_raster import dev_raster, dev_raster_runs  # noqa: E402
from test_gpu_regions import dev_regions  # noqa: E402
from test_gpu_runs import dev_runs  # noqa: E402
from test_gpu_shapes import dev_shapes  # noqa: E402
from test_gpu_simplify import dev_simplify  # noqa: E402

from infur_amd import _lib  # noqa: E402
from infur_amd.processors import Context  # noqa: E402

pytestmark = pytest.mark.gpu

TARGET = R.smooth(13, 70, seed=5, classes=5, cell=4)
TARGET_LOOPS = O.outline(TARGET, O.CONN8)
TARGET_SKIP = O.outline(TARGET, O.SKIP, 0)
TARGET_RUNS = RR.encode(TARGET, RR.SKIP, 0)
OVERLAP = A.loops_of([(3, A.rect(0, 0, 40, 9)), (200, A.rect(20, 4, 70, 13)), (90, A.rect(30, 2, 50, 6)[::-1])], 70)


def target_calls(ctx):
    """-> the bytes of every output of the small calls"""
    out = {}
    for tag, (l, v, c), kw in (("all ", TARGET_LOOPS, {}), ("skip ", TARGET_SKIP, dict(fill=0)), ("overlap ", OVERLAP, dict(fill=9)),
                               ("u32 ", TARGET_SKIP, dict(dtype=np.uint32, fill=0xFFFFFFFF)), ("cut ", TARGET_LOOPS, dict(loops_rows_in=len(TARGET_LOOPS[0]) - 1))):
        got = dev_raster(ctx, l, v, c, 13, 70, **kw)
        out.update({tag + name: got[name].tobytes() for name in ("plane", "counts")})
    got = dev_raster_runs(ctx, TARGET_RUNS[0], TARGET_RUNS[2], 13, 70)
    out.update({"runs " + name: got[name].tobytes() for name in ("plane", "counts")})
    return out


def reference():
    out = {}
    for tag, (l, v, c), kw in (("all ", TARGET_LOOPS, {}), ("skip ", TARGET_SKIP, {}), ("overlap ", OVERLAP, dict(fill=9)),
                               ("u32 ", TARGET_SKIP, dict(dtype=np.uint32, fill=0xFFFFFFFF))):
        plane, counts = A.raster(l, v, c, 13, 70, **kw)
        out.update({tag + "plane": plane.tobytes(), tag + "counts": counts.tobytes()})
    plane, counts = A.raster_runs(TARGET_RUNS[0], TARGET_RUNS[2], 13, 70)
    out.update({"runs plane": plane.tobytes(), "runs counts": counts.tobytes()})
    return out


@pytest.fixture(scope="module")
def fresh():
    assert _lib.load().infur_features() & _lib.FEATURE_RASTER  # (fails on a library without the feature)
    with Context(device=0) as c:
        got = target_calls(c)
    for name, want in reference().items():
        assert got[name] == want, name
    assert got["all plane"] == TARGET.tobytes()
    return got


def test_after_larger_and_denser_calls_of_the_same_stage(fresh):
    board = R.checkerboard(65, 129)
    bl, bv, bc = O.outline(board)
    stacked = A.loops_of([(250, A.rect(0, 0, 300, 40))] * 5 + [(7, A.rect(10, 5, 200, 30)[::-1])] * 3, 300)
    with Context(device=0) as c:
        dev_raster(c, bl, bv, bc, 65, 129)  # a larger plane, every pixel side a crossing
        dev_raster(c, *stacked, 40, 300, np.uint32, 5)  # windings of 5 and -3: words far from zero in every pixel
        dev_raster(c, bl, bv, bc, 65, 129, vertex_rows_in=len(bv) - 1)  # truncated: cleared, then nothing
        r, _, n = RR.encode(board)
        dev_raster_runs(c, r, n, 65, 129)
        dev_raster_runs(c, np.concatenate([r, r]), 2 * n, 65, 129)  # every run twice: every pixel a conflict
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
        dev_shapes(c, ol, ov, oc, 40, 130, rows=7)
        got = target_calls(c)
        dev_simplify(c, ol, ov, oc, 40, 130, 16)  # and they still work behind it
        assert np.frombuffer(got["all counts"], np.uint32)[0] == TARGET_LOOPS[2][0]
    for name in fresh:
        assert got[name] == fresh[name], name
