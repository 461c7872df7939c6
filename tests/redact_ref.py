"""Redact's rule (include/infur_hip.h) in numpy: int64 cumulative sums over the selected pixels, a box per pixel.  No product code."""
import numpy as np

FILL, PIXELATE, BLUR = 0, 1, 2
C_SELECTED, C_OUTSIDE, C_PASSES, C_STATUS = 0, 1, 2, 7
NOTHING = 1


def selection(plane, select, invert=False):
    """-> (selected [h, w] bool, the number of pixels whose value lies beyond the table)"""
    v = np.asarray(plane).astype(np.int64)
    select = np.asarray(select, np.uint8)
    inside = v < len(select)
    sel = np.zeros(v.shape, bool)
    sel[inside] = select[v[inside]] != 0
    return sel != bool(invert), int((~inside).sum())


def one_pass(pic, sel, y0, y1, x0, x1):
    """every selected pixel: per channel the mean over the selected pixels of its box rows [y0, y1), columns [x0, x1)"""
    h, w = sel.shape
    vals = np.concatenate([pic.astype(np.int64) * sel[..., None], sel[..., None].astype(np.int64)], axis=2)
    table = np.zeros((h + 1, w + 1, 4), np.int64)
    table[1:, 1:] = vals.cumsum(0).cumsum(1)
    box = table[y1, x1] - table[y0, x1] - table[y1, x0] + table[y0, x0]
    n = np.maximum(box[..., 3:], 1)  # (an unselected pixel's box may hold nothing; its result is not used)
    out = pic.copy()
    out[sel] = ((2 * box[..., :3] + n) // (2 * n))[sel].astype(np.uint8)
    return out


def redact(frame, plane, select, mode, size=0, passes=1, colour=0, invert=False):
    """-> (out [h, w, 3] u8, counts [8] u32)"""
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2]
    sel, outside = selection(plane, select, invert)
    yy, xx = np.mgrid[0:h, 0:w]
    out = frame.copy()
    done = 0
    if mode == FILL:
        out[sel] = [colour & 255, (colour >> 8) & 255, (colour >> 16) & 255]
    elif mode == PIXELATE:
        y0, x0 = yy - yy % size, xx - xx % size
        out = one_pass(out, sel, y0, np.minimum(y0 + size, h), x0, np.minimum(x0 + size, w))
        done = 1
    else:
        for _ in range(passes):
            out = one_pass(out, sel, np.maximum(yy - size, 0), np.minimum(yy + size + 1, h), np.maximum(xx - size, 0), np.minimum(xx + size + 1, w))
        done = passes
    n = int(sel.sum())
    return out, np.array([n, outside, done, 0, 0, 0, 0, 0 if n else NOTHING], np.uint32)

