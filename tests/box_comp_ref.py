"""A grid composite through the area-average pass (asciichat_hip_box_composites, include/asciichat_hip.h) restated in NumPy
over box_ref alone: tiles, the canvas under the renderers' cell lookup, the canvas averaged.  The box rule itself is stated in
box_ref.py and nowhere here.  TESTS ONLY."""
import numpy as np

import box_ref as BR


def tiles_ref(comp, images):
    """step 1: {k: source k averaged to tile_w x tile_h, no flips} for every placed source (k < n_src, src set).
    comp: anything with achip_composite_t's fields (the ctypes struct); images[k]: (src_h, src_w, 3) uint8 or None"""
    out = {}
    for k in range(comp.n_src):
        s = comp.s[k]
        if s.src:
            assert images[k].shape[:2] == (s.src_h, s.src_w)
            out[k] = BR.box_ref(images[k], s.tile_w, s.tile_h)
    return out


def canvas_ref(comp, tiles):
    """step 2: the canvas_h x canvas_w canvas, pixel by pixel as sample_composite finds it, a tile in place of the fetch"""
    canvas = np.zeros((comp.canvas_h, comp.canvas_w, 3), dtype=np.uint8)
    if comp.cell_w <= 0 or comp.cell_h <= 0:
        return canvas
    for Y in range(comp.canvas_h):
        row = Y // comp.cell_h
        if row >= comp.rows:
            continue
        for X in range(comp.canvas_w):
            col = X // comp.cell_w
            if col >= comp.cols:
                continue
            k = row * comp.cols + col
            if k >= comp.n_src or k not in tiles:
                continue
            s = comp.s[k]
            lx, ly = X - s.org_x, Y - s.org_y
            if 0 <= lx < s.tile_w and 0 <= ly < s.tile_h:
                canvas[Y, X] = tiles[k][ly, lx]
    return canvas


def composite_ref(comp, images, out_w, out_h, flip_x=False, flip_y=False):
    """steps 1-3: the averaged image of a composite frame, rounded twice by definition"""
    return BR.box_ref(canvas_ref(comp, tiles_ref(comp, images)), out_w, out_h, flip_x, flip_y)
