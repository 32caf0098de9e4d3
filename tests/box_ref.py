"""The area-average downscale (asciichat_hip_box_*, include/asciichat_hip.h) restated in NumPy, independent of the kernel and
of the host C: a plain loop over boxes.  TESTS ONLY."""
import numpy as np


def bounds(src, out, i):
    """the box of output index i on an axis of `src` pixels averaged to `out`: source indices lo .. hi - 1"""
    lo = i * src // out
    return lo, max(lo + 1, (i + 1) * src // out)


def box_ref(img, out_w, out_h, flip_x=False, flip_y=False):
    """img: (src_h, src_w, 3) uint8 -> (out_h, out_w, 3) uint8: per channel (S + n // 2) // n over each box, then the flips
    applied to the averaged image"""
    img = np.asarray(img, dtype=np.uint8)
    src_h, src_w = img.shape[:2]
    a = np.empty((out_h, out_w, 3), dtype=np.uint8)
    for y in range(out_h):
        y0, y1 = bounds(src_h, out_h, y)
        cols = img[y0:y1].sum(axis=0, dtype=np.int64)  # (src_w, 3)
        for x in range(out_w):
            x0, x1 = bounds(src_w, out_w, x)
            n = (x1 - x0) * (y1 - y0)
            a[y, x] = (cols[x0:x1].sum(axis=0) + n // 2) // n
    if flip_y:
        a = a[::-1]
    if flip_x:
        a = a[:, ::-1]
    return np.ascontiguousarray(a)


def box_ref_integer_factor(img, out_w, out_h):
    """the same for sources that are whole multiples of the averaged size, by reshape(...).sum(): a cross-check of the loop"""
    img = np.asarray(img, dtype=np.uint8)
    src_h, src_w = img.shape[:2]
    fy, fx = src_h // out_h, src_w // out_w
    assert fy * out_h == src_h and fx * out_w == src_w
    s = img.reshape(out_h, fy, out_w, fx, 3).astype(np.int64).sum(axis=(1, 3))
    n = fx * fy
    return ((s + n // 2) // n).astype(np.uint8)
