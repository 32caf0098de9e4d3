"""NumPy restatement of the grid-tile pass (include/asciichat_yuvgrid.h) over yuv_ref.py, independent of yuvgrid_math.h: the tile
a composite slot samples of a YUV source, where the tiles lie in their slab, and what a rewritten slot holds.  TESTS ONLY."""
from types import SimpleNamespace

import yuv_ref as YR

IDENTITY = 65537


def ratio(src_side, tile_side):
    """the reference's ratio of a src_side source resized to tile_side: ((s << 16) / d) + 1"""
    return (src_side << 16) // tile_side + 1


def tile(src, tile_w, tile_h, x_ratio, y_ratio):
    """-> [tile_h, tile_w, 3]: pixel (lx, ly) is the conversion of source pixel (min((lx * x_ratio) >> 16, width - 1),
    min((ly * y_ratio) >> 16, height - 1)) -- the composite samplers' lookup, which knows no flips"""
    return YR.sample(src, SimpleNamespace(src_w=src.width, src_h=src.height, out_w=tile_w, out_h=tile_h, x_ratio=x_ratio, y_ratio=y_ratio, ops=0))


def tile_bytes(tile_w, tile_h):
    return (3 * tile_w * tile_h + 15) // 16 * 16


def layout(sizes):
    """sizes: [(tile_w, tile_h)] of the YUV slots in order -> ([offset of tile t], the slab's bytes)"""
    at, pos = [], 0
    for tw, th in sizes:
        at.append(pos)
        pos += tile_bytes(tw, th)
    return at, (pos + 127) // 128 * 128


SLOT_FIELDS = ("src", "src_w", "src_h", "src_stride", "_pad0", "tile_w", "tile_h", "org_x", "org_y", "x_ratio", "y_ratio")
COMP_FIELDS = ("canvas_w", "canvas_h", "cols", "rows", "cell_w", "cell_h", "n_src", "_pad")


def rewritten_slot(slot, address):
    """the fields of a YUV slot after the rewrite, as a dict: the tile as an identity source, tile_* and org_* kept"""
    d = {f: getattr(slot, f) for f in SLOT_FIELDS}
    d.update(src=address, src_w=slot.tile_w, src_h=slot.tile_h, src_stride=3 * slot.tile_w, x_ratio=IDENTITY, y_ratio=IDENTITY)
    return d
