"""Anchors (a distance transform by value, one interior point per value) without a GPU: the ABI surface, the reference the GPU
tests use (tests/anchors_ref.py) against two independent restatements, hand-written answers and its own invariants, the caption
records of infur_amd.processors and the command line's argument errors."""
import ctypes as C
import io
import os
import re
import sys
from contextlib import redirect_stderr

import numpy as np
import pytest

from infur_amd import _lib, segments_cli
from infur_amd.processors import region_summary

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchors_ref as A  # noqa: E402
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_anchors", "infur_anchors_dev", "infur_frame_anchors", "infur_frame_anchors_dev")
CONSTANTS = {"INFUR_ANCHORS_SKIP": 1, "INFUR_ANCHOR_PIXEL": 0, "INFUR_ANCHOR_DIST2": 1, "INFUR_ANCHOR_WORDS": 2, "INFUR_FEATURE_ANCHORS": 256}
SMALL = ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (40, 70))


def families(h, w):
    yield "smooth", R.smooth(h, w, seed=h + w)
    yield "noise2", R.noise(h, w, 2, seed=w)
    yield "noise21", R.noise(h, w, 21, seed=h)
    yield "single", R.single(h, w)
    yield "vstripes", R.stripes(h, w, vertical=True)
    yield "hstripes", R.stripes(h, w, vertical=False)
    yield "checkerboard", R.checkerboard(h, w)
    yield "staircase", R.staircase(h, w)
    yield "disc", A.disc(h, w)
    yield "annulus", A.disc(h, w, annulus=True)
    yield "c", A.letter_c(max(h, 16), max(w, 16))


def skips(plane):
    """no skip, then the first pixel's value, the last pixel's and, for u32, 0xFFFFFFFF"""
    yield 0, 0
    for v in sorted({int(plane[0, 0]), int(plane[-1, -1])} | ({0xFFFFFFFF} if plane.dtype == np.uint32 else set())):
        yield A.SKIP, v


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_ANCHORS
    assert _lib.FEATURE_ANCHORS == 256 and lib.infur_features() & 255 == 255  # the eight older bits stay set
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    assert "pub struct HipAnchors" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Anchors" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def _args(text, at):
    """the top-level arguments of the call or declaration whose opening parenthesis is text[at]"""
    depth, cur, out = 0, "", []
    for ch in text[at:]:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                return out + ([cur.strip()] if cur.strip() else [])
        if ch == "," and depth == 1:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    raise AssertionError("unbalanced call")


def test_the_rust_wrapper_call_matches_the_declaration():
    """the wrapper crate is not compiled by this suite: its call passes as many arguments as the sys crate declares, and every
    sys constant it names exists"""
    sys_rs = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    wrapper = open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    decl, call = re.search(r"pub fn infur_anchors\s*\(", sys_rs), re.search(r"sys::infur_anchors\s*\(", wrapper)
    assert decl and call
    assert len(_args(wrapper, call.end() - 1)) == len(_args(sys_rs, decl.end() - 1)) == 10
    body = wrapper[wrapper.index("pub struct Anchors {"):wrapper.index("// ---------------------------------------------------------------- Outlines")]
    assert "impl Processor for HipAnchors" in body and "pub enum AnchorsCmd" in body
    for name in set(re.findall(r"sys::(INFUR_[A-Z0-9_]+)", body)):
        assert re.search(r"pub const %s\s*:" % name, sys_rs), name
    assert body.count("{") == body.count("}") and body.count("(") == body.count(")")


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert re.search(r"#define\s+INFUR_ANCHOR_NONE\s+0xFFFFFFFFu", header) and _lib.ANCHOR_NONE == 0xFFFFFFFF == A.NONE
    assert (A.SKIP, A.PIXEL, A.DIST2, A.WORDS) == (_lib.ANCHORS_SKIP, _lib.ANCHOR_PIXEL, _lib.ANCHOR_DIST2, _lib.ANCHOR_WORDS)


def test_rejected_calls_need_no_gpu(lib):
    """Every rejected call of the header's list is INFUR_E_INVALID_ARG on a host without a device, where the only context there
    can be is none, and no output is touched.  (The order of the checks shows in the messages of a live context:
    tests/test_gpu_anchors.py.)"""
    ow, oh, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(77)
    buf = np.full(4096, 0xA5, np.uint8)
    p = buf.ctypes.data
    for fn in (lib.infur_anchors, lib.infur_anchors_dev):
        for elem, hh, ww, flags, skip, plane, dist2, anchors, rows in (
                (1, 2, 2, 2, 0, p, p, p, 4),          # an unknown flag bit
                (1, 2, 2, 1, 256, p, p, p, 4),        # skip_value > 255 with 1-byte elements
                (2, 2, 2, 0, 0, p, p, p, 4),          # any other elem_bytes
                (4, 65536, 1, 0, 0, p, p, p, 4),      # h above 65535
                (4, 1, 65536, 0, 0, p, p, p, 4),      # w above 65535
                (4, 2, 2, 0, 0, None, p, p, 4),       # a NULL plane with h * w > 0
                (4, 2, 2, 0, 0, p, None, None, 4),    # nothing wanted
                (4, 2, 2, 0, 0, p, None, p, 0),       # a table without rows is not wanted
                (4, 2, 2, 1, 9, p, p, p, 4)):         # (and a good call: there is no context)
            assert fn(None, plane, elem, hh, ww, flags, skip, dist2, anchors, rows) == _lib.E_INVALID_ARG
    assert lib.infur_frame_anchors(None, p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, p, 64, p, 4, C.addressof(n), None, C.byref(ow), C.byref(oh),
                                   p, 64, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_anchors_dev(None, p, 4, 4, 1.0, 0, 0, 8, 0, 0, None, None, 0, p, 64, p, 4, p, None, C.byref(ow), C.byref(oh), p, 64,
                                       p) == _lib.E_INVALID_ARG
    assert n.value == 77 and (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


# ---------------------------------------------------------------- the reference
def test_the_three_references_agree():
    for h, w in SMALL:
        for name, k in families(h, w):
            for plane in (k, U.as_u32(k)):
                for flags, skip_value in skips(plane):
                    d = A.distance(plane, flags, skip_value)
                    assert d.dtype == np.uint32 and d.shape == plane.shape
                    assert (d == A.distance_brute(plane, flags, skip_value)).all(), (name, h, w, plane.dtype, flags, skip_value)
                    assert (d == A.distance_scipy(plane, flags, skip_value)).all(), (name, h, w, plane.dtype, flags, skip_value)


def test_the_letter_c():
    c = A.letter_c()
    ys, xs = np.nonzero(c == 1)
    assert (xs.mean(), ys.mean()) == (10.0, 11.5) and c[11, 10] == 0  # the centroid of class 1 is a pixel of class 0
    d = A.distance(c, A.SKIP, 0)
    rows = A.anchors(c, d, 3)
    assert rows.tolist() == [[A.NONE, 0], [4 * 24 + 4, 9], [A.NONE, 0]]  # (x 4, y 4): the centre line of the 5-wide upper arm
    assert c[4, 4] == 1
    # without the skip the background is a region too: its most interior pixel is in the notch
    d0 = A.distance(c, 0, 0)
    rows0 = A.anchors(c, d0, 2)
    assert (d0[c == 1] == d[c == 1]).all() and rows0[1].tolist() == rows[1].tolist()
    assert c.ravel()[rows0[0, A.PIXEL]] == 0 and rows0[0, A.DIST2] == d0[c == 0].max() == 25


def test_hand_written_planes():
    assert A.distance(np.array([[5]], np.uint8)).tolist() == [[1]]
    assert A.distance(R.single(1, 5)).tolist() == [[1, 1, 1, 1, 1]] and A.distance(R.single(5, 1)).ravel().tolist() == [1] * 5
    assert A.distance(R.single(5, 5)).tolist() == [[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 4, 9, 4, 1], [1, 4, 4, 4, 1], [1, 1, 1, 1, 1]]
    p = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]], np.uint8)
    assert A.distance(p).tolist() == [[1, 1, 1, 1], [1, 4, 1, 1], [1, 4, 2, 1], [1, 4, 4, 1], [1, 1, 1, 1]]  # 2: the nearest differing pixel is diagonal
    assert A.distance(p, A.SKIP, 1).tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert A.anchors(p, A.distance(p), 3).tolist() == [[7, 1], [5, 4], [A.NONE, 0]]  # ties go to the smallest index
    assert A.anchors(p, A.distance(p, A.SKIP, 1), 2).tolist() == [[7, 1], [A.NONE, 0]]  # the skipped value has no row
    assert A.anchors(p, A.distance(p), 1).tolist() == [[7, 1]] and A.anchors(p, A.distance(p), 0).shape == (0, 2)
    q = np.array([[0xFFFFFFFF, 7, 7]], np.uint32)
    assert A.distance(q, A.SKIP, 0xFFFFFFFF).tolist() == [[0, 1, 1]] and A.anchors(q, A.distance(q), 8).tolist() == [[A.NONE, 0]] * 7 + [[1, 1]]
    for h, w in ((0, 4), (3, 0), (0, 0)):  # the empty plane: the NONE rows and nothing else
        e = np.zeros((h, w), np.uint8)
        assert A.distance(e).shape == (h, w) and A.anchors(e, A.distance(e), 2).tolist() == [[A.NONE, 0]] * 2


def test_reference_invariants():
    for h, w in SMALL + ((135, 241),):
        for name, k in families(h, w):
            for flags, skip_value in skips(k):
                d = A.distance(k, flags, skip_value).astype(np.int64)
                kept = (k != skip_value) if flags else np.ones(k.shape, bool)
                assert ((d >= 1) == kept).all() and (d[~kept] == 0).all(), name  # dist2 >= 1 exactly off the skipped pixels
                hh, ww = k.shape
                edge = np.zeros(k.shape, bool)
                edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
                assert (d[edge & kept] == 1).all(), name  # a pixel that touches the frame
                rows = A.anchors(k, d, 22)
                yy, xx = np.mgrid[0:hh, 0:ww]
                for v, (at, d2) in enumerate(rows.tolist()):
                    here = kept & (k == v)
                    assert (at == A.NONE) == (not here.any()), (name, v)
                    if at == A.NONE:
                        assert d2 == 0
                        continue
                    y, x = divmod(at, ww)
                    assert k[y, x] == v and d2 == d[y, x] == d[here].max() and at == np.flatnonzero((d == d2).ravel() & here.ravel())[0]
                    # the disc of radius sqrt(DIST2) - 1 around the anchor: inside the value, and inside the picture
                    r = np.sqrt(d2) - 1
                    disc = (yy - y) ** 2 + (xx - x) ** 2 <= r * r
                    assert (k[disc] == v).all() and x - r >= 0 and y - r >= 0 and x + r <= ww - 1 and y + r <= hh - 1, (name, v)
    assert A.distance(R.single(135, 241)).max() == 68 * 68  # a run across four waves of 64 columns


# ---------------------------------------------------------------- the caption records
def test_region_summary_without_anchors_is_what_it_was():
    table = np.zeros((2, _lib.REGION_WORDS), np.uint64)
    table[0, [_lib.STAT_PIXELS, _lib.STAT_SUM_X, _lib.STAT_SUM_Y, _lib.STAT_MAX_X, _lib.STAT_MAX_Y, _lib.REGION_CLASS, _lib.REGION_FIRST]] = [4, 6, 2, 2, 1, 15, 1]
    table[1, [_lib.STAT_PIXELS, _lib.STAT_SUM_X, _lib.STAT_SUM_Y, _lib.STAT_MAX_X, _lib.STAT_MAX_Y, _lib.REGION_CLASS, _lib.REGION_FIRST]] = [1, 3, 3, 3, 3, 0, 15]
    names = ["background"] + ["x"] * 14 + ["person"]
    plain = region_summary(table, 2, 4, 4, names)
    assert [sorted(r) for r in plain] == [["box", "centroid", "first", "id", "klass", "mean_confidence", "name", "pixels", "share"]] * 2
    assert repr(plain) == repr(region_summary(table, 2, 4, 4, names, anchors=None))  # byte for byte
    with_a = region_summary(table, 2, 4, 4, names, anchors=np.array([[5, 2], [A.NONE, 0]], np.uint32))
    assert with_a[0]["anchor"] == [1, 1] and with_a[0]["radius"] == 1.41 and with_a[1]["anchor"] is None and with_a[1]["radius"] is None
    for r, q in zip(plain, with_a):
        assert all(q[key] == val for key, val in r.items())
    short = region_summary(table, 2, 4, 4, names, anchors=np.zeros((1, 2), np.uint32))  # fewer anchor rows than table rows
    assert short[0]["anchor"] == [0, 0] and short[1]["anchor"] is None


# ---------------------------------------------------------------- the command line
@pytest.mark.parametrize("argv,message", [
    (["--anchors"], "--anchors needs --regions or --tracks"),
    (["--regions", "--dist-out", "d.u32"], "--dist-out needs --anchors"),
    (["--dist-out", "d.u32"], "--dist-out needs --anchors"),
])
def test_cli_argument_errors(argv, message):
    err = io.StringIO()
    with pytest.raises(SystemExit) as e, redirect_stderr(err):
        segments_cli.main(["--width", "8", "--height", "8", "--synthetic-weights"] + argv)
    assert e.value.code == 2 and message in err.getvalue()


def test_rate_script_tables_without_a_device(capsys):
    """scripts/anchors_rate.py imports, generates its planes and formats both tables (made-up times: only the code path is checked)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("anchors_rate", os.path.join(ROOT, "scripts", "anchors_rate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dry-run"])
    lines = capsys.readouterr().out.splitlines()
    assert sum(line.startswith("| smooth") or line.startswith("| one class") or line.startswith("| noise") for line in lines) == 3
    assert sum(line.startswith("| f32 r50") for line in lines) == 3 == sum(line.startswith("| f16hl r50") for line in lines)  # three legs each
    assert all(line.count("|") >= 5 for line in lines if line.startswith("|"))
