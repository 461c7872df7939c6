"""Segments (class plane, softmax confidence, per-class statistics) without a GPU: the ABI surface, the reference the GPU tests
use (tests/segments_ref.py) against the reference's known-answer tests, and the band condition of the softmax inputs."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("infur_features", "infur_voc_class_name", "infur_segments", "infur_segments_dev", "infur_frame_segments",
               "infur_frame_segments_dev")
CONSTANTS = {"INFUR_DECODE_RAW": 0, "INFUR_DECODE_SOFTMAX": 1, "INFUR_STAT_PIXELS": 0, "INFUR_STAT_SUM_X": 1, "INFUR_STAT_SUM_Y": 2,
             "INFUR_STAT_SUM_CONF": 3, "INFUR_STAT_MIN_X": 4, "INFUR_STAT_MIN_Y": 5, "INFUR_STAT_MAX_X": 6, "INFUR_STAT_MAX_Y": 7,
             "INFUR_STAT_WORDS": 8, "INFUR_FEATURE_SEGMENTS": 1}


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"{s} is not exported"
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} is not declared in include/infur_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        assert re.search(r"pub fn %s\s*\(" % s, rust), f"{s} is not bound in rust/infur-hip-sys"
    assert lib.infur_abi_version() == 7 == _lib.ABI_VERSION  # the addition is announced by the feature bit, not the version
    assert lib.infur_features() & _lib.FEATURE_SEGMENTS


def test_constants_agree_in_header_binding_and_crate():
    header = open(os.path.join(ROOT, "include", "infur_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "infur-hip-sys", "src", "lib.rs")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == val, name
        m = re.search(r"pub const %s\s*:\s*u32\s*=\s*(\d+)\s*;" % name, rust)
        assert m and int(m.group(1)) == val, name
        assert getattr(_lib, name[len("INFUR_"):]) == val, name
        assert getattr(R, name[len("INFUR_"):].replace("DECODE_", "").replace("STAT_", ""), val) == val


def test_voc_class_names(lib):
    assert lib.infur_voc_class_name(0) == b"__background__"
    assert lib.infur_voc_class_name(15) == b"person"
    assert lib.infur_voc_class_name(20) == b"tvmonitor"
    assert lib.infur_voc_class_name(21) is None and lib.infur_voc_class_name(0xFFFFFFFF) is None
    assert len({lib.infur_voc_class_name(k) for k in range(21)}) == 21


def test_argument_errors_need_no_gpu(lib):
    """a null context is refused before anything else, like every other entry point"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    buf = np.zeros(64, np.uint8)
    assert lib.infur_segments(None, buf.ctypes.data, 1, 4, 4, 0, buf.ctypes.data, None, None, None) == _lib.E_INVALID_ARG
    assert lib.infur_segments_dev(None, None, 1, 4, 4, 0, None, None, None, None) == _lib.E_INVALID_ARG
    assert lib.infur_frame_segments(None, buf.ctypes.data, 4, 4, 1.0, 0, 0, buf.ctypes.data, None, 16, None, 0, None, 0, None,
                                    C.byref(ow), C.byref(oh)) == _lib.E_INVALID_ARG


def test_raw_reference_is_the_oracles_argmax(oracle, kats):
    rng = np.random.default_rng(11)
    for k, h, w in ((21, 33, 47), (1, 4, 4), (40, 7, 9)):
        x = rng.normal(0.4, 0.5, size=(k, h, w)).astype(np.float32)
        x[rng.random(x.shape) < 0.01] = np.nan
        x[rng.random(x.shape) < 0.01] = np.inf
        x[rng.random(x.shape) < 0.01] = -np.inf
        kl, cf = R.decode(x, R.RAW, oracle)
        ok, oc = oracle.argmax(x)
        assert (kl == ok).all() and (cf == oc).all()
        # ... and the loop it restates, spelled out: first strict maximum above 0.0, NaN never wins
        cand = np.where(np.isnan(x), -np.inf, x)
        best = cand.max(axis=0)
        want_k = np.where(best > 0, cand.argmax(axis=0), 0)
        want_c = R.as_u8(np.where(best > 0, best, 0).astype(np.float32) * np.float32(255.0))
        assert (kl == want_k).all() and (cf == want_c).all()
    # decode_0to1 (decode_predict.rs:100-116): every pixel class 21, confidence non-decreasing, last 255
    kat = kats["decode_0to1"]
    hm = np.linspace(0.0, 1.0, kat["linspace"][2], dtype=np.float32).reshape(kat["shape"])
    kl, cf = R.decode(hm, R.RAW, oracle)
    assert kl.shape == (kat["height"], kat["width"]) and (kl == kat["klass"]).all()
    assert (np.diff(cf.ravel().astype(int)) >= 0).all() and cf.ravel()[-1] == kat["last_alpha"]
    st = R.stats(kl, cf, kat["shape"][0])
    assert st[kat["klass"], R.PIXELS] == kat["height"] * kat["width"] and st[0, R.PIXELS] == 0 and st[0, R.MIN_X] == R.U64_MAX
    # color_2 (decode_predict.rs:94-97): class 2 at 0.5 -> 127
    one = np.zeros((3, 1, 1), np.float32)
    one[2] = kats["color_2"]["alpha"]
    kl, cf = R.decode(one, R.RAW, oracle)
    assert kl[0, 0] == kats["color_2"]["klass"] and cf[0, 0] == kats["color_2"]["unmultiplied_rgba"][3] == 127


def test_softmax_reference_on_crafted_values():
    inf, nan = np.inf, np.nan
    px = np.array([
        [nan, nan, nan],        # nothing wins: class 0, conf 0
        [-inf, -inf, -inf],     # the same
        [1.0, inf, 2.0],        # +inf: class 1, conf 255
        [nan, -3.0, nan],       # NaN beside a finite maximum: class 1, p = 1
        [-2.0, -2.0, -5.0],     # negative logits are legitimate maxima; the first maximum wins
        [0.0, 0.0, 0.0],        # p = 1/3 -> 85
        [-inf, 7.0, -inf],      # -inf terms contribute 0: p = 1
    ], np.float32).T.reshape(3, 1, 7)
    kl, cf = R.decode(px, R.SOFTMAX)
    assert kl.ravel().tolist() == [0, 0, 1, 1, 0, 0, 1]
    p = 1.0 / (2.0 + np.exp(-3.0))
    assert cf.ravel().tolist() == [0, 0, 255, 255, int(np.float32(np.float32(p) * np.float32(255.0))), 85, 255]
    st = R.stats(kl, cf, 3)
    assert st[0].tolist() == [4, 0 + 1 + 4 + 5, 0, int(cf.ravel()[[0, 1, 4, 5]].astype(int).sum()), 0, 0, 5, 0]
    assert st[2].tolist() == [0, 0, 0, 0, int(R.U64_MAX), int(R.U64_MAX), 0, 0]


def softmax_inputs(sigma, k, n):
    """the inputs of the GPU softmax test: N(0, sigma) logits from default_rng(5)"""
    return np.random.default_rng(5).normal(0.0, sigma, size=(k, n // 400, 400)).astype(np.float32)


@pytest.mark.parametrize("k", [21, 22])
@pytest.mark.parametrize("sigma", [1.0, 2.0, 4.0])
def test_softmax_inputs_keep_out_of_the_truncation_band(sigma, k):
    """conf = trunc(p * 255): where the exact product lies within 2e-3 of an integer an f32 evaluation may land on the other side,
    and the GPU test allows +-1 there.  An f32 evaluation of p carries about (K + 3) roundings of 2^-24 plus the exponent
    argument's |c - c_max| * 2^-24 per term: below 8e-6 relative for these inputs, times 255 -- so 2e-3 is a safe band, and
    the inputs must leave at most 1 % of the pixels inside it for the exact comparison to mean something."""
    x = softmax_inputs(sigma, k, 200_000)
    share = R.in_band(x).mean()
    print(f"sigma {sigma} K {k}: {100 * share:.2f} % of {x.shape[1] * x.shape[2]} pixels in the band")
    assert share <= 0.01
    # an f32 emulation of the kernel's formulation (sequential f32 sum of exp2 of the scaled difference) agrees outside the band
    kl, cf = R.decode(x, R.SOFTMAX)
    cmax = x.max(axis=0)
    s = np.zeros(cmax.shape, np.float32)
    for c in x:
        s = s + np.exp2(((c - cmax) * np.float32(1.44269504088896341)).astype(np.float32)).astype(np.float32)
    emu = R.as_u8((np.float32(1.0) / s) * np.float32(255.0))
    diff = emu.astype(int) - cf.astype(int)
    assert (diff[~R.in_band(x)] == 0).all() and (np.abs(diff) <= 1).all()


def test_class_summary_records():
    from infur_amd.processors import class_summary

    kl = np.zeros((4, 6), np.uint8)
    kl[1:3, 2:5] = 15
    cf = np.full((4, 6), 51, np.uint8)
    cf[kl == 15] = 255
    recs = class_summary(R.stats(kl, cf, 21), 6, 4)
    assert [r["name"] for r in recs] == ["__background__", "person"]
    person = recs[1]
    assert person["pixels"] == 6 and person["share"] == 0.25 and person["box"] == (2, 1, 4, 2)
    assert person["centroid"] == (3.0, 1.5) and person["mean_confidence"] == 1.0
    assert abs(recs[0]["mean_confidence"] - 0.2) < 1e-12
    assert class_summary(R.stats(kl, cf, 21), 6, 4, names=["bg"])[1]["name"] == "class15"
