"""NumPy restatement of the packed RGB tile passes (include/asciichat_pixgrid.h), independent of pixgrid.h and of the kernels: the
tile a composite slot samples of a packed source -- pix_ref's whole conversion, indexed by the composite samplers' rule --, the
averaged tile -- box_ref over the whole conversion --, where the tiles lie in their slab, and what a rewritten slot holds.
TESTS ONLY."""
import numpy as np

from box_ref import box_ref

IDENTITY = 65537


def ratio(src_side, tile_side):
    """the reference's ratio of a src_side source resized to tile_side: ((s << 16) / d) + 1"""
    return (src_side << 16) // tile_side + 1


def tile(img, tile_w, tile_h, x_ratio, y_ratio):
    """img: the whole conversion (pix_ref.whole) -> [tile_h, tile_w, 3]: pixel (lx, ly) is source pixel
    (min((lx * x_ratio) >> 16, w - 1), min((ly * y_ratio) >> 16, h - 1)), the products taken in 32 bits; no flips"""
    h, w = img.shape[:2]
    sx = [min(((lx * x_ratio) & 0xFFFFFFFF) >> 16, w - 1) for lx in range(tile_w)]
    sy = [min(((ly * y_ratio) & 0xFFFFFFFF) >> 16, h - 1) for ly in range(tile_h)]
    return np.ascontiguousarray(img[sy][:, sx])


def box_tile(img, tile_w, tile_h):
    """img: the whole conversion -> [tile_h, tile_w, 3]: its box average, no flips; the ratios play no part"""
    return box_ref(img, tile_w, tile_h, False, False)


def tile_bytes(tile_w, tile_h):
    return -(-3 * tile_w * tile_h // 16) * 16


def layout(sizes):
    """sizes: [(tile_w, tile_h)] of the packed slots in order -> ([offset of tile t], the slab's bytes: 0 without tiles)"""
    at, pos = [], 0
    for tw, th in sizes:
        at.append(pos)
        pos += tile_bytes(tw, th)
    return at, -(-pos // 128) * 128


SLOT_FIELDS = ("src", "src_w", "src_h", "src_stride", "_pad0", "tile_w", "tile_h", "org_x", "org_y", "x_ratio", "y_ratio")
COMP_FIELDS = ("canvas_w", "canvas_h", "cols", "rows", "cell_w", "cell_h", "n_src", "_pad")


def rewritten_slot(slot, address):
    """the fields of a packed slot after the rewrite, as a dict: the tile as an identity source, tile_* and org_* kept"""
    d = {f: getattr(slot, f) for f in SLOT_FIELDS}
    d.update(src=address, src_w=slot.tile_w, src_h=slot.tile_h, src_stride=3 * slot.tile_w, x_ratio=IDENTITY, y_ratio=IDENTITY)
    return d
