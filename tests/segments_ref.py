"""Reference of the Segments decode for the tests (numpy only; no product code).

Semantics, per output pixel over the K class values c_k in class order (include/infur_hip.h):

RAW      the reference's loop (decode_predict.rs:67-78): k_max = 0, c_max = 0.0, strict '>';
         conf = (c_max * 255.0) as u8, saturating and truncating.  Taken from the C oracle (``COracle.argmax``).
SOFTMAX  the same loop from c_max = -inf: NaN never wins, the first maximum wins.
         p = 1 / sum_k exp(c_k - c_max) over the K classes, NaN terms contributing 0;
         c_max still -inf: class 0, conf 0;  c_max = +inf: conf 255;  otherwise conf = (p * 255.0) as u8.
         Computed here in float64, then p is rounded to f32, the f32 product p * 255 is taken, truncated and saturated.

Statistics per class k < K, eight uint64 words: PIXELS, SUM_X, SUM_Y, SUM_CONF, MIN_X, MIN_Y, MAX_X, MAX_Y with x the
column and y the row; a class without a pixel reads 0, 0, 0, 0, UINT64_MAX, UINT64_MAX, 0, 0.
"""
import numpy as np

RAW, SOFTMAX = 0, 1
PIXELS, SUM_X, SUM_Y, SUM_CONF, MIN_X, MIN_Y, MAX_X, MAX_Y, WORDS = range(9)
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
BAND = 2e-3  # |p64 * 255 - nearest integer| below which an f32 evaluation may legitimately truncate to the other side


def as_u8(x32: np.ndarray) -> np.ndarray:
    """Rust ``as u8`` of an f32 array: NaN -> 0, saturate, truncate."""
    x = np.nan_to_num(x32.astype(np.float64), nan=0.0, posinf=255.0, neginf=0.0)
    return np.clip(np.trunc(x), 0, 255).astype(np.uint8)


def softmax_p64(khw: np.ndarray):
    """-> (klass [H,W] u8, p64 [H,W] f64, cmax [H,W] f64) of the SOFTMAX decode in float64; p64 is NaN where cmax is infinite"""
    c = np.asarray(khw, np.float32).astype(np.float64)
    k, h, w = c.shape
    if k == 0:
        return np.zeros((h, w), np.uint8), np.full((h, w), np.nan), np.full((h, w), -np.inf)
    cand = np.where(np.isnan(c), -np.inf, c)
    klass = np.argmax(cand, axis=0)  # the first maximum
    cmax = np.take_along_axis(cand, klass[None], axis=0)[0]
    klass = np.where(cmax == -np.inf, 0, klass).astype(np.uint8)  # strict '>' against -inf: nothing won
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(c - cmax[None])
        e = np.where(np.isnan(e), 0.0, e)
        s = e.sum(axis=0)
        p = np.where(np.isfinite(cmax), 1.0 / np.where(s > 0, s, 1.0), np.nan)
    return klass, p, cmax


def decode(khw: np.ndarray, mode: int, oracle=None):
    """-> (klass [H,W] u8, conf [H,W] u8)"""
    if mode == RAW:
        assert oracle is not None, "the RAW decode is the C oracle's oracle_argmax"
        k, h, w = khw.shape
        if k == 0 or h * w == 0:
            return np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        return oracle.argmax(np.ascontiguousarray(khw, np.float32))
    klass, p, cmax = softmax_p64(khw)
    p32 = np.where(np.isfinite(cmax), p, 0.0).astype(np.float32)
    conf = as_u8(p32 * np.float32(255.0))
    conf = np.where(cmax == np.inf, 255, np.where(cmax == -np.inf, 0, conf)).astype(np.uint8)
    return klass, conf


def in_band(khw: np.ndarray) -> np.ndarray:
    """[H,W] bool: pixels whose exact p * 255 lies within BAND of an integer (SOFTMAX; finite maxima only)"""
    _, p, cmax = softmax_p64(khw)
    v = np.where(np.isfinite(cmax), p, 0.5 / 255.0) * 255.0
    return np.isfinite(cmax) & (np.abs(v - np.round(v)) < BAND)


def stats(klass: np.ndarray, conf: np.ndarray, k: int) -> np.ndarray:
    """-> [k, 8] uint64 from a class plane and a confidence plane"""
    h, w = klass.shape
    out = np.zeros((k, 8), np.uint64)
    out[:, MIN_X] = U64_MAX
    out[:, MIN_Y] = U64_MAX
    if k == 0 or h * w == 0:
        return out
    kl = klass.astype(np.int64).ravel()
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    out[:, PIXELS] = np.bincount(kl, minlength=k)[:k].astype(np.uint64)
    for col, wt in ((SUM_X, xs), (SUM_Y, ys), (SUM_CONF, conf.astype(np.int64).ravel())):
        out[:, col] = np.round(np.bincount(kl, weights=wt.astype(np.float64), minlength=k)[:k]).astype(np.uint64)  # < 2^53: exact
    for c in np.unique(kl):
        m = kl == c
        out[c, MIN_X], out[c, MAX_X] = xs[m].min(), xs[m].max()
        out[c, MIN_Y], out[c, MAX_Y] = ys[m].min(), ys[m].max()
    return out
