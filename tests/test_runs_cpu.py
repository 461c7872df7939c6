"""Runs (a plane as run-length records) without a GPU: the ABI surface, the reference the GPU tests use (tests/runs_ref.py)
against hand-written answers and its own invariants, and the decoders of infur_amd.processors."""
import ctypes as C
import os
import re
import sys

import numpy as np

from infur_amd import _lib
from infur_amd.processors import runs_by_value, runs_decode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import runs_ref as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_runs", "infur_runs_dev", "infur_frame_runs", "infur_frame_runs_dev")
CONSTANTS = {"INFUR_RUNS_SKIP": 1, "INFUR_RUN_START": 0, "INFUR_RUN_END": 1, "INFUR_RUN_VALUE": 2, "INFUR_RUN_WORDS": 3, "INFUR_FEATURE_RUNS": 8}


def planes():
    for h, w in ((1, 1), (1, 5), (5, 1), (3, 64), (7, 65), (33, 63), (2, 130), (135, 241)):
        yield "smooth", R.smooth(h, w, seed=h)
        yield "noise2", R.noise(h, w, 2, seed=w)
        yield "noise21", R.noise(h, w, 21, seed=w)
        yield "single", R.single(h, w)
        yield "single0", R.single(h, w, c=0)
        yield "vstripes", R.stripes(h, w, vertical=True)
        yield "hstripes", R.stripes(h, w, vertical=False)
        yield "checkerboard", R.checkerboard(h, w)
        yield "staircase", R.staircase(h, w)


def test_symbols_are_declared_exported_and_bound(lib):
    """fails on a library without the feature: this is the test that proves it"""
    assert lib.infur_features() & _lib.FEATURE_RUNS
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    assert lib.infur_features() & _lib.FEATURE_TRACKS and lib.infur_features() & _lib.FEATURE_REGIONS and lib.infur_features() & _lib.FEATURE_SEGMENTS
    assert "pub struct HipRuns" in open(os.path.join(ROOT, "rust", "infur-hip", "src", "lib.rs")).read()
    assert "class Runs" in open(os.path.join(ROOT, "include", "infur_processor.hpp")).read()


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
    assert (U.SKIP, U.START, U.END, U.VALUE, U.WORDS) == (_lib.RUNS_SKIP, _lib.RUN_START, _lib.RUN_END, _lib.RUN_VALUE, _lib.RUN_WORDS)


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else and no output is touched"""
    ow, oh, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(77)
    buf = np.full(256, 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.infur_runs(None, p, 1, 2, 2, 0, 0, p, 4, p, C.addressof(n)) == _lib.E_INVALID_ARG
    assert lib.infur_runs_dev(None, p, 4, 2, 2, 1, 9, p, 4, p, p) == _lib.E_INVALID_ARG
    assert lib.infur_frame_runs(None, p, 4, 4, 1.0, 0, 0, 0, 0, p, 4, p, 5, C.addressof(n), None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert lib.infur_frame_runs_dev(None, p, 4, 4, 1.0, 0, 0, 0, 0, p, 4, p, 5, p, None, 0, None, C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG
    assert n.value == 77 and (buf == 0xA5).all() and (ow.value, oh.value) == (0, 0)


# ---------------------------------------------------------------- the reference against hand-written answers
def test_reference_on_hand_written_planes():
    p = np.array([[1, 1, 2, 2, 2], [2, 0, 0, 3, 3]], np.uint8)  # the 2 that ends row 0 and the 2 that begins row 1 are two runs
    runs, rs, n = U.encode(p)
    assert n == 5 and runs.tolist() == [[0, 2, 1], [2, 5, 2], [5, 6, 2], [6, 8, 0], [8, 10, 3]] and rs.tolist() == [0, 2, 5]
    runs, rs, n = U.encode(p, U.SKIP, 2)
    assert n == 3 and runs.tolist() == [[0, 2, 1], [6, 8, 0], [8, 10, 3]] and rs.tolist() == [0, 1, 3]
    runs, rs, n = U.encode(p, 0, 2)  # the flag is what skips, not the value
    assert n == 5
    q = np.array([[0xFFFFFFFF, 0xFFFFFFFF, 1 << 30]], np.uint32)
    runs, rs, n = U.encode(q, U.SKIP, 0xFFFFFFFF)
    assert n == 1 and runs.tolist() == [[2, 3, 1 << 30]] and rs.tolist() == [0, 1]
    runs, rs, n = U.encode(np.full((3, 4), 9, np.uint8), U.SKIP, 9)  # everything skipped
    assert n == 0 and runs.shape == (0, 3) and rs.tolist() == [0, 0, 0, 0]
    for h, w in ((0, 4), (3, 0), (0, 0)):  # the empty plane: no run, every row starts at 0
        runs, rs, n = U.encode(np.zeros((h, w), np.uint8))
        assert n == 0 and runs.shape == (0, 3) and rs.tolist() == [0] * (h + 1)


def test_reference_invariants_and_round_trip():
    counts = {}
    for name, k in planes():
        h, w = k.shape
        for plane, dtype in ((k, np.uint8), (U.as_u32(k), np.uint32)):
            runs, rs, n = U.encode(plane)
            U.check_invariants(runs, rs, n, h, w, skipping=False)
            assert (U.decode(runs, n, h, w, 0, dtype) == plane).all(), (name, h, w)
            assert (runs_decode(runs, n, h, w, dtype=dtype) == plane).all(), (name, h, w)  # the product's decoder
            counts[(name, h, w)] = n
            for skip in sorted({int(plane[0, 0]), int(plane[-1, -1]), 5}):
                sruns, srs, sn = U.encode(plane, U.SKIP, skip)
                U.check_invariants(sruns, srs, sn, h, w, skipping=True)
                assert sn == n - int((runs[:, U.VALUE] == skip).sum()) and (sruns == runs[runs[:, U.VALUE] != skip]).all()
                assert (U.decode(sruns, sn, h, w, skip, dtype) == plane).all(), (name, h, w, skip)
                assert (runs_decode(sruns, sn, h, w, fill=skip, dtype=dtype) == plane).all(), (name, h, w, skip)
    assert counts[("single", 135, 241)] == 135 and counts[("hstripes", 135, 241)] == 135  # one run per row, never longer
    assert counts[("checkerboard", 135, 241)] == 135 * 241 == counts[("vstripes", 135, 241)]
    assert counts[("single", 1, 1)] == 1 and counts[("noise21", 5, 1)] == 5


def test_decoders_of_the_package():
    p = np.array([[1, 1, 2, 2, 2], [2, 0, 0, 3, 3]], np.uint8)
    runs, _, n = U.encode(p)
    assert runs_decode(runs, n, 2, 5).dtype == np.uint8 and (runs_decode(runs, n, 2, 5) == p).all()
    assert (runs_decode(runs, 2, 2, 5, fill=9) == np.array([[1, 1, 2, 2, 2], [9, 9, 9, 9, 9]])).all()  # a truncated table decodes to its prefix
    assert (runs_decode(runs[:0], 0, 2, 5, fill=4) == 4).all()
    by = runs_by_value(runs, n)
    assert sorted(by) == [0, 1, 2, 3] and by[2].tolist() == [[2, 5], [5, 6]] and by[3].tolist() == [[8, 10]]
    assert runs_by_value(runs, 0) == {}
    big = U.as_u32(p)
    bruns, _, bn = U.encode(big)
    out = runs_decode(bruns, bn, 2, 5, fill=0xFFFFFFFF)
    assert out.dtype == np.uint32 and (out == big).all()


def test_rate_script_tables_without_a_device(capsys):
    """scripts/runs_rate.py imports, generates its planes and formats both tables (made-up times: only the code path is checked)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("runs_rate", os.path.join(ROOT, "scripts", "runs_rate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--dry-run"])
    lines = capsys.readouterr().out.splitlines()
    assert sum(line.startswith("| smooth") or line.startswith("| one class") or line.startswith("| noise") for line in lines) == 6
    assert sum(line.startswith("| f32 r50") for line in lines) == 3 and all(line.count("|") >= 7 for line in lines if line.startswith("|"))
    klass = R.smooth(54, 96)
    assert f"| smooth 54x96 | u8 class | {U.encode(klass)[2]} |" in "\n".join(lines)
    assert mod.bytes_to_host("segments", 10, 4, 2, 5, 3) == 40 + 128 and mod.bytes_to_host("runs", 10, 4, 2, 5, 3) == 4 + 36 + 20 + 128
