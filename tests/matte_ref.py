"""Matte's and Composite's rules (include/infur_hip.h) in numpy int64: a shifted-slice loop over the window.  No product code."""
import numpy as np

from redact_ref import selection

INVERT, CONF = 1, 2
C_SELECTED, C_OUTSIDE, C_CLEAR, C_SOFT, C_OPAQUE, C_STATUS = 0, 1, 2, 3, 4, 7
NOTHING = 1
COLOUR, IMAGE, CUTOUT = 0, 1, 2


def weights(sigma):
    """weight(d) for d = 0 .. 765"""
    d = np.arange(766, dtype=np.int64)
    return (4096 * sigma * sigma) // (sigma * sigma + d * d)


def matte(frame, plane, select, radius, sigma, flags=0, conf=None):
    """-> (alpha [h, w] u8, counts [8] u32)"""
    f = np.asarray(frame, np.uint8).astype(np.int64)
    h, w = f.shape[:2]
    sel, outside = selection(plane, select, flags & INVERT)
    m = np.where(sel, np.asarray(conf, np.int64) if flags & CONF else 255, 0)
    wt = weights(sigma)
    N, D = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue  # no pixel has this tap inside the frame
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))  # the pixels p whose tap q = p + (dy, dx) lies inside
            yq, xq = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
            wgt = wt[np.abs(f[ys, xs] - f[yq, xq]).sum(axis=2)]
            D[ys, xs] += wgt
            N[ys, xs] += wgt * m[yq, xq]
    assert N.max() <= 1137438720 and (2 * N + D).max() < 1 << 32
    alpha = ((2 * N + D) // (2 * D)).astype(np.uint8)
    n = int(sel.sum())
    counts = [n, outside, int((alpha == 0).sum()), int(((alpha > 0) & (alpha < 255)).sum()), int((alpha == 255).sum()), 0, 0, 0 if n else NOTHING]
    return alpha, np.array(counts, np.uint32)


def composite(frame, alpha, mode, back=None, colour=0):
    """-> [h, w, 3] u8, or [h, w, 4] u8 for CUTOUT"""
    frame, alpha = np.asarray(frame, np.uint8), np.asarray(alpha, np.uint8)
    if mode == CUTOUT:
        return np.concatenate([frame, alpha[..., None]], axis=2)
    under = np.asarray(back, np.int64) if mode == IMAGE else np.array([colour & 255, (colour >> 8) & 255, (colour >> 16) & 255], np.int64)
    a = alpha.astype(np.int64)[..., None]
    return ((a * frame.astype(np.int64) + (255 - a) * under + 127) // 255).astype(np.uint8)
