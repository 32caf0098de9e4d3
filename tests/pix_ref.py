"""The packed RGB sources of include/asciichat_pix.h restated in NumPy, independent of the kernels and of the host C: the whole
conversion by slicing, the sampled image by the descriptor's rule, the box image as box_ref over the whole conversion.
TESTS ONLY."""
import numpy as np

from box_ref import box_ref

RGB, RGBA, BGR, BGRA = 0, 1, 2, 3
FORMATS = (RGB, RGBA, BGR, BGRA)
NAMES = {RGB: "RGB", RGBA: "RGBA", BGR: "BGR", BGRA: "BGRA"}
BPP = {RGB: 3, RGBA: 4, BGR: 3, BGRA: 4}
ORDER = {RGB: (0, 1, 2), RGBA: (0, 1, 2), BGR: (2, 1, 0), BGRA: (2, 1, 0)}  # the bytes of a pixel that are R, G, B
FLIP_X, FLIP_Y = 1, 2


def whole(data, fmt, w, h, stride=0):
    """data: the source's bytes from its pixel (0, 0) on (1-D uint8) -> (h, w, 3) RGB24"""
    bpp = BPP[fmt]
    stride = stride or bpp * w
    rows = np.stack([data[y * stride:y * stride + bpp * w] for y in range(h)]).reshape(h, w, bpp)
    return np.ascontiguousarray(rows[:, :, list(ORDER[fmt])])


def sample(img, f):
    """img: the whole conversion; f: a frame descriptor -> (out_h, out_w, 3): pixel (x, y) is source pixel
    sx = min((x * x_ratio) >> 16, w - 1), sy alike, then the flips of ops"""
    h, w = img.shape[:2]
    sx = np.minimum((np.arange(f.out_w, dtype=np.uint64) * f.x_ratio & 0xFFFFFFFF) >> 16, w - 1).astype(np.int64)
    sy = np.minimum((np.arange(f.out_h, dtype=np.uint64) * f.y_ratio & 0xFFFFFFFF) >> 16, h - 1).astype(np.int64)
    if f.ops & FLIP_X:
        sx = w - 1 - sx
    if f.ops & FLIP_Y:
        sy = h - 1 - sy
    return np.ascontiguousarray(img[sy][:, sx])


def box(img, out_w, out_h, flip_x=False, flip_y=False):
    return box_ref(img, out_w, out_h, flip_x, flip_y)
