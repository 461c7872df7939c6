"""The cases of tests/test_gpu_decode_heads.py, checked without a GPU: tests/heads.py's restatement of the form selection against
prepost.hip, the case table against the forms it must reach, and the REFERENCE's own figures for every case -- the share of pixels
in the confidence band (float64 / integer forward here, the GPU test repeats it on its own logits), and that the crafted heads do
produce what they are for (all-negative pixels, twins that win, non-finite values, exact ties), so that no GPU case is vacuous.

Low-res logits here: oracle.TorchModel in float64 up to ``classifier.0`` (one forward per frame; the backbone does not depend on the
head), the 1x1 head in float64, rounded to f32; quantised models: oracle/infur_qoracle.py.  From there the chain is the GPU test's."""
import os
import re
import sys

import numpy as np
import pytest

from infur_amd import weights as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads as H  # noqa: E402
import segments_ref as R  # noqa: E402


# ---- 1. form selection ---------------------------------------------------------------------------------------------------------------
def test_form_constants_match_the_sources():
    src = open(os.path.join(H.ROOT, "infur_amd", "csrc", "prepost.hip")).read()
    m = re.search(r"constexpr int UP_TW = (\d+), UP_TH = (\d+), UP_KP = (\d+);", src)
    assert m and tuple(int(v) for v in m.groups()) == (H.UP_TW, H.UP_TH, H.UP_KP) == (64, 16, 24)
    body = re.search(r"static size_t up_tile_lds_bytes\(int LH, int LW, int K, int OH, int OW\) \{(.*?)\n\}", src, re.S).group(1)
    assert "if (K > UP_KP || K <= 0 || OH <= 0 || OW <= 0) return 0;" in body
    assert f"const size_t cols = (size_t)(((long long)UP_TW * LW + OW - 1) / OW) + {H.UP_HALO};" in body
    assert f"const size_t rows = (size_t)(((long long)UP_TH * LH + OH - 1) / OH) + {H.UP_HALO};" in body
    assert "const size_t bytes = (UP_TW + UP_TH) * sizeof(Lerp) + rows * cols * UP_KP * sizeof(float);" in body
    assert "return bytes <= 48 * 1024 ? bytes : 0;" in body and H.UP_LDS_LIMIT == 48 * 1024 and H.UP_HALO == 3
    # sizeof(Lerp): two ints and two floats, nothing else
    lerp = re.search(r"struct Lerp \{(.*?)\};", src, re.S).group(1).split()
    assert lerp == ["int", "i1,", "i2;", "float", "d1,", "d2;"] and H.LERP_BYTES == 16
    # the seven-way switch: 0 = scalar, 1..5 by number, everything else <6>; on ceil(K / 4) where the footprint fits
    macro = re.search(r"#define UP_LAUNCH\(STAGED, SCALAR, \.\.\.\)(.*?)while \(0\)", src, re.S).group(1)
    assert "const size_t lds = up_tile_lds_bytes(LH, LW, K, OH, OW);" in macro and "switch (lds ? (K + 3) / 4 : 0) {" in macro
    labels = re.findall(r"(case \d+|default): hipLaunchKernelGGL\((SCALAR|STAGED<(\d)>), (rows|tiles), dim3\(256\), (0|lds), s,", macro)
    assert [(a, b) for a, b, *_ in labels] == [("case 0", "SCALAR")] + [(f"case {n}", f"STAGED<{n}>") for n in range(1, 6)] + [("default", "STAGED<6>")]
    assert all((grid, lds) == (("rows", "0") if kern == "SCALAR" else ("tiles", "lds")) for _, kern, _, grid, lds in labels)
    # every decode product goes through this launcher pair
    assert "UP_LAUNCH(upsample_argmax_segments_lds_kernel, upsample_argmax_segments_kernel, low, LH, LW, K, softmax, lut, o, OH, OW, uq);" in src
    assert H.UP_MAX_PIXELS == 498


def test_up_form_edges():
    assert [H.up_form(7, 13, k, 52, 100) for k in (1, 4, 5, 8, 9, 20, 21, 24)] == [1, 1, 2, 2, 3, 5, 6, 6]
    assert H.up_form(7, 13, 25, 52, 100) == 0 and H.up_form(7, 13, 0, 52, 100) == 0 and H.up_form(7, 13, 256, 52, 100) == 0
    assert H.up_form(7, 13, 21, 0, 100) == 0
    # the limit itself: 498 staged pixels fit, 499 do not (the rule is on bytes; K does not enter the footprint)
    assert (H.UP_TW + H.UP_TH) * H.LERP_BYTES + 498 * 96 <= H.UP_LDS_LIMIT < (H.UP_TW + H.UP_TH) * H.LERP_BYTES + 499 * 96
    # the network's own ratio: 1080p stages 5 x 11 pixels
    lh, lw = W.lowres_dims(1080, 1920)
    assert H.up_footprint(lh, lw, 1080, 1920) == 55 and H.up_form(lh, lw, 21, 1080, 1920) == 6


def test_case_table_reaches_every_form():
    table = H.case_table()
    for head, ks in (("float", H.FLOAT_KS), ("quant", H.QUANT_KS)) + tuple((hd, H.CRAFTED_KS) for hd in H.CRAFTED_HEADS):
        forms = {(k, s): f for hd, k, s, f in table if hd == head}
        assert {k for k, _ in forms} == set(ks)
    fl = {(k, s): f for hd, k, s, f in table if hd == "float"}
    # every staged instantiation, at every multi-tile size; both residues' pad counts at more than one NQ
    for s in ((52, 100), (50, 99), (17, 65), (9, 9), (4, 1), (1, 3)):
        assert {fl[k, s] for k in H.FLOAT_KS if k <= 24} == {1, 2, 3, 4, 5, 6}, s
        assert all(fl[k, s] == (k + 3) // 4 for k in H.FLOAT_KS if k <= 24), s
        assert all(fl[k, s] == 0 for k in (25, 31)), s  # scalar by class count
    for r in range(4):
        assert len({(k + 3) // 4 for k in H.FLOAT_KS if k <= 24 and k % 4 == r}) >= 2, r
    # scalar by footprint, at every class count
    for s in ((3, 1), (1, 2), (2, 1), (1, 1)):
        assert all(fl[k, s] == 0 for k in H.FLOAT_KS), s
    # the footprints of the tiny sizes, and the two sides of the limit one step apart
    for s, n in H.FOOTPRINTS.items():
        lh, lw = W.lowres_dims(*s)
        assert (lh, lw) == (1, 1) and H.up_footprint(lh, lw, s[0], s[1]) == n and (n <= H.UP_MAX_PIXELS) == (fl[20, s] != 0), s
    for staged, scalar in H.BOUNDARY_PAIRS:
        assert abs(staged[0] - scalar[0]) + abs(staged[1] - scalar[1]) == 1
        assert H.FOOTPRINTS[staged] <= H.UP_MAX_PIXELS < H.FOOTPRINTS[scalar]
        for k in H.FLOAT_KS:
            assert fl[k, staged] == ((k + 3) // 4 if k <= 24 else 0) and fl[k, scalar] == 0, (k, staged, scalar)
    # the sizes' other properties: dword / byte stores, a second tile row and column with one live pixel, low-res 2 x 2
    assert 100 % 4 == 0 and 99 % 4 and 52 % H.UP_TH and (17, 65) == (H.UP_TH + 1, H.UP_TW + 1) and W.lowres_dims(9, 9) == (2, 2)
    # crafted heads: pads of every residue but 0 (K = 5, 22, 23), scalar (26), and both sides of the limit
    cr = {(k, s): f for hd, k, s, f in table if hd == "negative"}
    assert {cr[k, (52, 100)] for k in H.CRAFTED_KS} == {2, 6, 0} and sorted(k % 4 for k in H.CRAFTED_KS if k <= 24) == [1, 2, 3]
    assert all(cr[k, (1, 3)] == ((k + 3) // 4 if k <= 24 else 0) and cr[k, (1, 2)] == 0 for k in H.CRAFTED_KS)
    qu = {(k, s): f for hd, k, s, f in table if hd == "quant"}
    assert [qu[k, (52, 100)] for k in H.QUANT_KS] == [2, 6, 0] and all(qu[k, (1, 2)] == 0 for k in H.QUANT_KS)
    assert set(H.GUARD_SIZES) <= set(H.SIZES)


def test_the_heads_are_the_synthetic_models():
    """heads.py builds every model from one cached set of tensors: the blobs are W.synth_blob's byte for byte"""
    for k in (5, 31):
        assert H.float_blob(k) == W.synth_blob(num_classes=k, aux=False)
    assert H.twin_pairs(5) == [(0, 1), (3, 4)] and H.twin_pairs(22) == [(0, 1), (3, 4), (9, 14), (20, 21)]
    assert H.twin_pairs(23)[-1] == (21, 22) and H.twin_pairs(26)[-1] == (24, 25)
    w, b = H.crafted_head("twins", 22)
    assert all((w[i] == w[j]).all() and b[i] == b[j] for i, j in H.twin_pairs(22)) and len({bytes(r) for r in w.reshape(22, -1)}) == 18
    w, b = H.crafted_head("nonfinite", 5)
    assert b[2] == np.inf and np.isnan(b[1]) and b[4] == -np.inf and np.isfinite(w).all()
    meta, tensors = W.unpack_blob(H.crafted_blob("nonfinite", 5))  # the format carries them unchanged
    assert meta["num_classes"] == 5 and not meta["aux"] and H.same_floats(np.array(tensors[-1][2]), b)


# ---- 2. the reference's own figures ----------------------------------------------------------------------------------------------------
class Features:
    """classifier.0's output in float64 per (frame index, size): the input of every head of that frame"""

    def __init__(self, oracle):
        from oracle.infur_oracle import TorchModel

        self.oracle = oracle
        self.model = TorchModel(H.float_blob(1), float64=True)
        self.cache = {}

    def __call__(self, K, size):
        if (K, size) not in self.cache:
            taps = {}
            self.model.forward_lowres(self.oracle.pack_normalize(H.frame(K, size)), taps)
            self.cache[K, size] = taps["classifier.0"].numpy()
        return self.cache[K, size]

    def ref(self, K, size, head):
        """the reference of the case whose classifier.4 is head = (weight, bias)"""
        w, b = head
        feat = self(K, size)
        with np.errstate(invalid="ignore"):
            lo = np.einsum("kc,chw->khw", w.reshape(K, -1).astype(np.float64), feat) + b.astype(np.float64)[:, None, None]
        return H.Ref(self.oracle.upsample_bilinear(lo.astype(np.float32), size[0], size[1]), self.oracle)


@pytest.fixture(scope="module")
def features(oracle):
    return Features(oracle)


def pooled_band(refs):
    return sum(int(r.band.sum()) for r in refs) / sum(r.band.size for r in refs)


def test_float_models_stay_under_the_band_cap(features):
    shares = {}
    for k in H.FLOAT_KS:
        head = H.float_tensors(k)[-1][1:]
        refs = [features.ref(k, s, head) for s in H.SIZES]
        shares[k] = pooled_band(refs)
        assert all((r.sm_klass < k).all() for r in refs)
        if k == 1:
            assert all((r.sm_conf == 255).all() and r.band.all() for r in refs)  # p = 1: 255 exactly, which is why K = 1 is exempt
    print("in-band share per K:", {k: f"{100 * v:.2f} %" for k, v in shares.items()})
    assert all(v <= H.BAND_CAP for k, v in shares.items() if k >= 2), shares


def test_crafted_heads_do_what_they_are_for(features):
    shares = {}
    for k in H.CRAFTED_KS:
        # all negative: every class value of every pixel is below zero, so RAW answers class 0 / conf 0 and SOFTMAX a real maximum
        refs = [features.ref(k, s, H.crafted_head("negative", k)) for s in H.CRAFTED_SIZES]
        shares["negative", k] = pooled_band(refs)
        for r in refs:
            assert (r.up < 0).all() and np.isfinite(r.up).all()
            assert (r.raw_klass == 0).all() and (r.raw_conf == 0).all() and r.raw_stats[0, R.PIXELS] == r.band.size
            assert (r.sm_klass == r.up.argmax(axis=0)).all() and (r.sm_klass < k).all()
        if k == 22:
            assert len(np.unique(refs[0].sm_klass)) == 7 and abs(refs[0].up.max() - -46.9) < 0.05
        assert len(np.unique(refs[0].sm_klass)) > 1  # a pad class that won would not hide behind a constant plane
        # twins: bit-equal planes; the earlier one wins, and does win somewhere
        pairs = H.twin_pairs(k)
        refs = [features.ref(k, s, H.crafted_head("twins", k)) for s in H.CRAFTED_SIZES]
        shares["twins", k] = pooled_band(refs)
        later = [j for _, j in pairs]
        for r in refs:
            assert all((r.up[i].view(np.uint32) == r.up[j].view(np.uint32)).all() for i, j in pairs)
            assert not np.isin(r.sm_klass, later).any() and not np.isin(r.raw_klass, later).any()
        wins = {i: int((refs[0].sm_klass == i).sum()) for i, _ in pairs}
        print(f"twins K {k}: pixels of 52x100 won by the earlier twins {wins}")
        assert sum(wins.values()) > 0, (k, wins)
        if k == 22:
            assert wins == {0: 0, 3: 216, 9: 0, 20: 650}, wins
        # non-finite: +inf wins the interior at 255, the border interpolates 0 * inf = NaN and falls back on the finite classes
        refs = [features.ref(k, s, H.crafted_head("nonfinite", k)) for s in H.CRAFTED_SIZES]
        shares["nonfinite", k] = pooled_band(refs)
        for r, s in zip(refs, H.CRAFTED_SIZES):
            assert np.isnan(r.up[1]).all() and not np.isnan(r.up[[0, 3]]).any()
            if W.lowres_dims(*s) != (1, 1):
                inner = r.up[2] == np.inf
                assert inner.any() and np.isnan(r.up[2]).any() and (inner | np.isnan(r.up[2])).all()
                assert (r.sm_klass[inner] == 2).all() and (r.sm_conf[inner] == 255).all() and (r.sm_klass[~inner] != 2).all()
                assert ((r.up[4] == -np.inf) == inner).all() and (r.raw_klass[inner] == 2).all() and (r.raw_conf[inner] == 255).all()
            assert not np.isin(r.sm_klass, (1, 4)).any()
    print("in-band share per crafted head:", {k: f"{100 * v:.2f} %" for k, v in shares.items()})
    assert all(v <= H.BAND_CAP for v in shares.values()), shares


def test_quantised_heads_tie_and_stay_under_the_band_cap(oracle):
    shares, ties = {}, {}
    for k in H.QUANT_KS:
        refs = {}
        for s in H.QUANT_SIZES:
            ups, _ = H.quant_reference_planes(k, s, oracle)
            assert ups[0].shape == (k,) + s and ups[1].shape == (k,) + s
            refs[s] = H.Ref(ups[0], oracle)
        shares[k] = pooled_band(list(refs.values()))
        for s in H.QUANT_LARGE:
            ties[k, s] = float(refs[s].top2_ties().mean())
    print("in-band share per quantised K:", {k: f"{100 * v:.2f} %" for k, v in shares.items()})
    print("exact top-2 ties:", {k: f"{100 * v:.2f} %" for k, v in ties.items()})
    assert all(v <= H.BAND_CAP for v in shares.values()), shares
    assert all(v >= 0.005 for v in ties.values()), ties
