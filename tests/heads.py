"""Helper of tests/test_gpu_decode_heads.py and tests/test_decode_heads_cpu.py (a plain module, no tests): which form of the fused
up-sampling kernels a geometry takes, the table of (head, class count, size) cases that reaches every form, the models with another
class count or a rewritten ``classifier.4``, and the reference of one fused decode with the rules it is compared by.

The fused decode is graded given the run's OWN low-res logits (the conv stack is graded elsewhere), so the reference chain is
``oracle.upsample_bilinear(lo, h, w)`` -> ``segments_ref.decode`` -> ``segments_ref.stats`` and ``oracle.colorcode`` for the mask.
"""
import functools
import os
import sys

import numpy as np

from infur_amd import weights as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segments_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- form selection: prepost.hip's up_tile_lds_bytes and the UP_LAUNCH switch, restated ---------------------------------------------
UP_TW, UP_TH, UP_KP = 64, 16, 24  # output tile, floats of a staged pixel slot
UP_HALO = 3                       # the "+ 3" of the staged rectangle's rows and columns
UP_LDS_LIMIT = 48 * 1024
LERP_BYTES = 16                   # sizeof(Lerp): two ints, two floats
# the most rows x cols of staged pixels that fit: (48 KB - 80 coordinates) / 96 bytes = 498
UP_MAX_PIXELS = (UP_LDS_LIMIT - (UP_TW + UP_TH) * LERP_BYTES) // (UP_KP * 4)


def up_footprint(LH, LW, OH, OW):
    """rows x cols of low-res pixels the staged kernels reserve for one 64 x 16 output tile"""
    cols = (UP_TW * LW + OW - 1) // OW + UP_HALO
    rows = (UP_TH * LH + OH - 1) // OH + UP_HALO
    return rows * cols


def up_lds_bytes(LH, LW, K, OH, OW):
    if K > UP_KP or K <= 0 or OH <= 0 or OW <= 0:
        return 0
    b = (UP_TW + UP_TH) * LERP_BYTES + up_footprint(LH, LW, OH, OW) * UP_KP * 4
    return b if b <= UP_LDS_LIMIT else 0


def up_form(LH, LW, K, OH, OW):
    """0: the scalar kernel; else NQ = ceil(K / 4) of the LDS-staged kernel (the switch's default label is 6)"""
    return min((K + 3) // 4, 6) if up_lds_bytes(LH, LW, K, OH, OW) else 0


def form_of(K, size):
    h, w = size
    lh, lw = W.lowres_dims(h, w)
    return up_form(lh, lw, K, h, w)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
FLOAT_KS = (1, 2, 3, 4, 5, 8, 11, 14, 17, 20, 23, 24, 25, 31)
SIZES = (
    (52, 100),  # dword stores of the byte planes; rows end inside a 16-row tile
    (50, 99),   # byte stores
    (17, 65),   # the second tile column and the second tile row hold one live pixel each
    (9, 9),     # low-res 2 x 2
    (4, 1),     # staged, every tile coordinate clamped: 469 staged pixels of at most 498
    (1, 3),     # the same, 475
    (3, 1),     # scalar by footprint: 603
    (1, 2),     # 665
    (2, 1),     # 737
    (1, 1),     # 1273
)
BOUNDARY_PAIRS = (((4, 1), (3, 1)), ((1, 3), (1, 2)))  # (staged, scalar): one step across the footprint limit
FOOTPRINTS = {(4, 1): 469, (1, 3): 475, (3, 1): 603, (1, 2): 665, (2, 1): 737, (1, 1): 1273}
GUARD_SIZES = ((50, 99), (17, 65))

CRAFTED_HEADS = ("negative", "twins", "nonfinite")
CRAFTED_KS = (5, 22, 23, 26)
CRAFTED_SIZES = ((52, 100), (50, 99), (17, 65), (1, 3), (1, 2))

QUANT_KS = (6, 21, 26)
QUANT_SIZES = ((52, 100), (50, 99), (1, 2))
QUANT_LARGE = ((52, 100), (50, 99))

BAND_CAP = 0.01  # share of a case's pixels (all its sizes pooled) that may lie in segments_ref.in_band: test_unfused_softmax's


def case_table():
    """every (head, K, size) that tests/test_gpu_decode_heads.py runs -> [(head, K, size, form)]"""
    out = [("float", k, s, form_of(k, s)) for k in FLOAT_KS for s in SIZES]
    out += [(hd, k, s, form_of(k, s)) for hd in CRAFTED_HEADS for k in CRAFTED_KS for s in CRAFTED_SIZES]
    out += [("quant", k, s, form_of(k, s)) for k in QUANT_KS for s in QUANT_SIZES]
    return out


def frame(K, size):
    return W.synth_frame(size[0], size[1], index=K)


# ---- the models ---------------------------------------------------------------------------------------------------------------------
_KMAX = max(FLOAT_KS + CRAFTED_KS)


@functools.lru_cache(maxsize=None)
def _base_tensors():
    """W.synth_tensors(50, _KMAX, False), made once: the generator draws every tensor from a counter stream of its own, so the
    backbone does not depend on the class count and the head of K classes is the first K rows of a larger one
    (test_decode_heads_cpu.py checks the blobs against W.synth_blob)"""
    return [(c.name, w, b) for c, w, b in W.synth_tensors(50, _KMAX, False)]


def float_tensors(K):
    """== list(W.synth_tensors(50, K, False)) with names for specs"""
    base = _base_tensors()
    name, w, b = base[-1]
    assert name == "classifier.4" and 1 <= K <= _KMAX
    return base[:-1] + [(name, w[:K], b[:K])]


def float_blob(K):
    """== W.synth_blob(num_classes=K, aux=False)"""
    return W.pack_blob(float_tensors(K), 50, K, False)


def twin_pairs(K):
    """(earlier, later) class pairs with identical classifier rows, those that fit K classes"""
    pairs = []
    for i, j in ((0, 1), (3, 4), (9, 14), (K - 2, K - 1)):
        if 0 <= i < j < K and not any(i in p or j in p for p in pairs):
            pairs.append((i, j))
    return pairs


def crafted_head(head, K):
    """classifier.4 of the K-class synthetic model, rewritten -> (weight [K,512,1,1] f32, bias [K] f32).  The base of all three:
    weights x 3 (logits that differ by more than the synthetic model's few tenths) and the 0.01 * k trend of the biases removed (no
    class is favoured by its index)."""
    _, w, b = float_tensors(K)[-1]
    w = (w * np.float32(3.0)).astype(np.float32)
    b = (b.astype(np.float64) - 0.01 * np.arange(K)).astype(np.float32)
    if head == "negative":
        b = b - np.float32(50.0)
    elif head == "twins":
        for i, j in twin_pairs(K):
            w[j], b[j] = w[i], b[i]
    elif head == "nonfinite":
        b[2], b[1], b[4] = np.inf, np.nan, -np.inf
    else:
        raise ValueError(head)
    return w, b


def crafted_blob(head, K):
    w, b = crafted_head(head, K)
    return W.pack_blob(float_tensors(K)[:-1] + [("classifier.4", w, b)], 50, K, False)


@functools.lru_cache(maxsize=None)
def quant_blobs(K):
    """-> (the statically quantised K-class model as quantize.synth_qblob makes it, the same model flagged as one whose file resizes
    the u8 codes of its heads before DequantizeLinear)"""
    from infur_amd import quantize

    frames = [quantize.normalise(W.synth_frame(96, 128, index=100 + k)) for k in range(3)]
    qblob = quantize.quantise_model(W.synth_blob(num_classes=K), frames)
    _, convs, adds = W.unpack_qblob(qblob)
    return qblob, W.pack_qblob(convs, adds, 50, K, True, resize_u8=True)


def quant_reference_planes(K, size, oracle):
    """the integer oracle's head codes, resized as u8 and dequantised -> ([out, aux] full-resolution f32 planes, dequantised low-res
    logits (out, aux))"""
    from oracle import infur_qoracle as Q

    h, w = size
    qblob, _ = quant_blobs(K)
    chw = oracle.pack_normalize(frame(K, size))
    codes, params = Q.qforward_codes(qblob, chw)
    ups = [Q.resize_u8_then_dequantise(cd, zp, sc, h, w, oracle.upsample_bilinear) for cd, (zp, sc) in zip(codes, params)]
    lows = [((cd - np.float32(zp)) * np.float32(sc)).astype(np.float32) for cd, (zp, sc) in zip(codes, params)]
    return ups, lows


# ---- the reference of one decode and the rules of the comparison ---------------------------------------------------------------------
class Ref:
    """everything the reference says about full-resolution class planes ``up`` [K,h,w] f32; computed once, never changed"""

    def __init__(self, up, oracle):
        self.up = up
        self.K = K = up.shape[0]
        self.raw_klass, self.raw_conf = R.decode(up, R.RAW, oracle)
        self.raw_stats = R.stats(self.raw_klass, self.raw_conf, K)
        self.sm_klass, self.sm_conf = R.decode(up, R.SOFTMAX)
        self.sm_stats = R.stats(self.sm_klass, self.sm_conf, K)
        self.band = R.in_band(up)
        self.mask = oracle.colorcode(up)

    def top2_ties(self):
        """[h,w] bool: the two largest class values of the pixel are equal (NaN sorts last and counts as no value)"""
        if self.K < 2:
            return np.zeros(self.up.shape[1:], bool)
        s = np.sort(np.where(np.isnan(self.up), -np.inf, self.up), axis=0)
        return (s[-1] == s[-2]) & (s[-1] > -np.inf)


EXACT_COLS = [R.PIXELS, R.SUM_X, R.SUM_Y, R.MIN_X, R.MIN_Y, R.MAX_X, R.MAX_Y]


def same_floats(a, b):
    """bit-equal, or NaN in both (the sign and payload of a NaN are not defined across host and device)"""
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_raw(ref, s, what):
    """RAW: class, confidence, statistics and overlay equal the reference"""
    assert s.klass.shape == ref.raw_klass.shape and s.stats.shape == (ref.K, 8), what
    assert (s.klass == ref.raw_klass).all(), (what, "klass", int((s.klass != ref.raw_klass).sum()))
    assert (s.conf == ref.raw_conf).all(), (what, "conf", int((s.conf != ref.raw_conf).sum()))
    assert (s.stats == ref.raw_stats).all(), (what, "stats")
    assert (s.rgba == ref.mask).all(), (what, "rgba")


def check_softmax(ref, s, lut, what):
    """SOFTMAX, by the rules of test_unfused_softmax: the class exact and < K; the confidence exact outside the band and within 1
    inside it; the statistics exact but for SUM_CONF, that within the class's in-band pixel count, and exact for the kernel's own
    planes; the overlay the LUT of the kernel's own planes"""
    K = ref.K
    assert s.klass.shape == ref.sm_klass.shape and s.stats.shape == (K, 8), what
    assert (s.klass < K).all(), (what, "a class index >= K", int(s.klass.max()))
    assert (s.klass == ref.sm_klass).all(), (what, "klass", int((s.klass != ref.sm_klass).sum()))
    diff = s.conf.astype(int) - ref.sm_conf.astype(int)
    assert (diff[~ref.band] == 0).all(), (what, "a confidence byte differs outside the band", int((diff[~ref.band] != 0).sum()))
    assert (np.abs(diff) <= 1).all(), (what, "conf", int(np.abs(diff).max()))
    assert (s.stats[:, EXACT_COLS] == ref.sm_stats[:, EXACT_COLS]).all(), (what, "stats")
    per_class = np.bincount(ref.sm_klass[ref.band].ravel(), minlength=K)
    dsum = np.abs(s.stats[:, R.SUM_CONF].astype(np.int64) - ref.sm_stats[:, R.SUM_CONF].astype(np.int64))
    assert (dsum <= per_class).all(), (what, "SUM_CONF")
    assert (s.stats == R.stats(s.klass, s.conf, K)).all(), (what, "stats of the kernel's own planes")
    assert (s.rgba == lut[s.klass % 20, s.conf]).all(), (what, "rgba")
    if K == 1:
        assert (s.conf == 255).all(), what
