"""The boundary families of the fused composite sampler (sample_composite, sample_composite_lds and their callers in the phase,
stream and rows kernels), shared by tests/test_composite_boundaries.py (CPU emulator) and tests/test_gpu_composite.py.  TESTS ONLY.

A case is a list of sources (numpy HxWx3 arrays; None = a client without video), a terminal size, and its PREMISE: what
achip_composite_setup must make of it (grid, cell size, placed tiles) and what the oracle's canvas must look like for the case
to test what its name says.  Where a premise does not hold the case is wrong, not the kernel.  Expectations come from the
oracle alone: orc.composite for the canvas, orc.convert_with_caps(canvas, W, h, cl, rm, True, True, False) for a frame
(h = 2 * th for the half-block render modes; the truecolor-background renderer, which no capability set maps to, is
orc.print_truecolor_bg over the oracle's resize of the canvas)."""
import ctypes as C

import numpy as np

import orc
from achip_ctypes import MODE_CAPS, MODE_TRUE_BG, Composite

S = (8, 6)  # the usual source: 4:3, a few pixels


class Case:
    def __init__(self, name, family, dims, term, grid, cell, tiles, n_src=None, canvas=None):
        """dims: [(w, h) | None]; term: (tw, th); grid: (cols, rows); cell: (cell_w, cell_h);
        tiles: per placed slot (tile_w, tile_h, org_x, org_y, index into dims) or None for a slot left empty (src == NULL);
        canvas: optional check(case, canvas, imgs) of the premise on the oracle's canvas"""
        self.name, self.family, self.dims, self.term = name, family, dims, term
        self.grid, self.cell, self.tiles = grid, cell, tiles
        self.n_src = len(tiles) if n_src is None else n_src
        self.canvas_check = canvas
        self._imgs = self._canvas = None
        self._exp = {}

    def __repr__(self):
        return self.name

    @property
    def imgs(self):
        if self._imgs is None:
            self._imgs = [None if d is None else orc.frame_hash_noise(d[0], d[1], 50 + i) for i, d in enumerate(self.dims)]
        return self._imgs

    @property
    def canvas_dims(self):
        return self.term[0], 2 * self.term[1]

    def canvas(self):
        """the oracle's canvas (computed once, never written), its premise asserted"""
        if self._canvas is None:
            cv = orc.composite(self.imgs, *self.term)
            cv.setflags(write=False)
            assert cv.shape == (2 * self.term[1], self.term[0], 3), (self.name, cv.shape)
            if self.canvas_check:
                self.canvas_check(self, cv, self.imgs)
            self._canvas = cv
        return self._canvas

    def frame_height(self, mode):
        return 2 * self.term[1] if MODE_CAPS.get(mode, (3, 0))[1] == 2 else self.term[1]

    def expected(self, mode):
        """the frame the oracle renders from its canvas (computed once per mode)"""
        if mode not in self._exp:
            tw, th = self.term
            if mode == MODE_TRUE_BG:
                # no capability set reaches this renderer: the canvas at the terminal's size, which is what the aspect rule
                # makes of a W x 2H canvas in a W x H terminal -- no padding
                assert orc.aspect_ratio(tw, 2 * th, tw, th, False) == (tw, th), self.name
                self._exp[mode] = orc.print_truecolor_bg(orc.resize_nn(self.canvas(), tw, th))
            else:
                cl, rm = MODE_CAPS[mode]
                self._exp[mode] = orc.convert_with_caps(self.canvas(), tw, self.frame_height(mode), cl, rm, True, True, False)
        return self._exp[mode]

    # ---- the descriptor ----------------------------------------------------------------------------------------
    def descriptor(self, L, addresses, cls=Composite):
        """achip_composite_setup over `addresses` (one per source: host memory for the emulator, device memory on the GPU;
        None / 0 where the source is None; cls: the structure class L's prototypes were declared with), premise asserted"""
        n = len(self.dims)
        assert len(addresses) == n
        ptrs = (C.c_void_p * n)(*[a if d is not None else None for a, d in zip(addresses, self.dims)])
        ws = (C.c_int * n)(*[0 if d is None else d[0] for d in self.dims])
        hs = (C.c_int * n)(*[0 if d is None else d[1] for d in self.dims])
        comp = cls()
        L.achip_composite_setup(C.byref(comp), ptrs, ws, hs, n, *self.term)
        self.check_premise(comp, addresses)
        return comp

    def host_descriptor(self, L):
        return self.descriptor(L, [None if i is None else i.ctypes.data for i in self.imgs])

    def check_premise(self, comp, addresses):
        name = self.name
        have = [d for d in self.dims if d is not None]
        assert (comp.canvas_w, comp.canvas_h) == self.canvas_dims, name
        assert (comp.cols, comp.rows) == self.grid, (name, comp.cols, comp.rows)
        assert (comp.cols, comp.rows) == orc.grid_layout(have, *self.term), (name, "the oracle's layout")
        assert (comp.cell_w, comp.cell_h) == self.cell, (name, comp.cell_w, comp.cell_h)
        assert comp.n_src == self.n_src == len(self.tiles), (name, comp.n_src)
        assert comp._pad == 0, name
        for k, t in enumerate(self.tiles):
            s = comp.s[k]
            if t is None:
                assert not s.src and (s.tile_w, s.tile_h) == (0, 0), (name, k, "an empty slot")
                continue
            tw, th, ox, oy, src = t
            assert (s.tile_w, s.tile_h, s.org_x, s.org_y) == (tw, th, ox, oy), (name, k, s.tile_w, s.tile_h, s.org_x, s.org_y)
            assert s.src == addresses[src] and (s.src_w, s.src_h) == self.dims[src] and s.src_stride == 3 * s.src_w, (name, k)
        for k in range(len(self.tiles), 9):
            assert not comp.s[k].src, (name, k)


def _tiles(cols, cell, tile, srcs):
    """equal tiles centred in their cells, slot k in cell (k % cols, k // cols)"""
    (cw, ch), (tw, th) = cell, tile
    return [(tw, th, (k % cols) * cw + (cw - tw) // 2, (k // cols) * ch + (ch - th) // 2, s) for k, s in enumerate(srcs)]


def _region(cv, t):
    tw, th, ox, oy = t[:4]
    return cv[oy:oy + th, ox:ox + tw]


# ---- premises on the oracle's canvas -------------------------------------------------------------------------------
def _all_black(case, cv, imgs):
    assert not cv.any(), case.name


def _tiles_lit_rest_black(case, cv, imgs):
    """every placed tile holds its source's resize; every pixel outside the tiles is black (margins, empty cells)"""
    mask = np.zeros(cv.shape[:2], bool)
    for t in case.tiles:
        if t is None:
            continue
        tw, th, ox, oy, src = t
        assert np.array_equal(_region(cv, t), orc.resize_nn(imgs[src], tw, th)), (case.name, src)
        assert _region(cv, t).any(), (case.name, src, "a noise tile is not black")
        mask[oy:oy + th, ox:ox + tw] = True
    assert not cv[~mask].any(), case.name


def _remainder(case, cv, imgs):
    """columns / rows behind the last cell exist and are black"""
    _tiles_lit_rest_black(case, cv, imgs)
    (cols, rows), (cw, ch), (W, H) = case.grid, case.cell, case.canvas_dims
    assert W % cols or H % rows, case.name
    if W % cols:
        assert cols * cw < W and not cv[:, cols * cw:].any(), case.name
    if H % rows:
        assert rows * ch < H and not cv[rows * ch:].any(), case.name


def _empty_trailing_cells(case, cv, imgs):
    _tiles_lit_rest_black(case, cv, imgs)
    (cols, rows), (cw, ch) = case.grid, case.cell
    assert case.n_src < cols * rows, case.name
    for k in range(case.n_src, cols * rows):
        x, y = (k % cols) * cw, (k // cols) * ch
        assert not cv[y:y + ch, x:x + cw].any(), (case.name, k)


def _margins(above_below):
    def check(case, cv, imgs):
        _tiles_lit_rest_black(case, cv, imgs)
        tw, th, ox, oy, _ = case.tiles[0]
        cw, ch = case.cell
        if above_below:
            assert tw == cw and ox == 0 and 0 < oy and oy + th < ch, case.name
        else:
            assert th == ch and oy == 0 and 0 < ox and ox + tw < cw, case.name
    return check


def _odd_margins(case, cv, imgs):
    _tiles_lit_rest_black(case, cv, imgs)
    cw, ch = case.cell
    assert any(t and ((cw - t[0]) % 2 or (ch - t[1]) % 2) for t in case.tiles), case.name


def _tile_is_cell(case, cv, imgs):
    _tiles_lit_rest_black(case, cv, imgs)
    assert all(t[:2] == case.cell for t in case.tiles) and cv.reshape(-1, 3).any(axis=1).all(), case.name


def _hole_in_the_middle(case, cv, imgs):
    _tiles_lit_rest_black(case, cv, imgs)
    hole = case.tiles.index(None)
    assert 0 < hole < len(case.tiles) - 1 and all(t is not None for t in case.tiles[hole + 1:]), case.name


def _one_pixel_sources(case, cv, imgs):
    """every tile of a 1x1 source is that pixel throughout"""
    _tiles_lit_rest_black(case, cv, imgs)
    seen = 0
    for t in case.tiles:
        if t and case.dims[t[4]] == (1, 1):
            assert (_region(cv, t) == imgs[t[4]][0, 0]).all(), case.name
            seen += 1
    assert seen, case.name


def _upscaled(case, cv, imgs):
    """several canvas pixels hit source pixel (0, 0) and the source's last pixel"""
    _tiles_lit_rest_black(case, cv, imgs)
    t = case.tiles[0]
    r, im = _region(cv, t), imgs[t[4]]
    assert (r[:2, :2] == im[0, 0]).all() and (r[-2:, -2:] == im[-1, -1]).all(), case.name


ALL_NONE = "only clients without video"
ZERO_CELL = "cell_h == 0: nine sources at 20x4"
ONE_PIXEL_CELL_H = "cell_h == 1: nine sources at 20x5"
ONE_PIXEL_CELLS = "cells of 1x1: nine sources at 1x5"


def cases():
    c = []
    # ---- grid fill: 1..9 equal sources at 60x30 (measured: 1x1, 1x2, 2x2, 2x3 and 3x3, columns x rows) ----------------
    fill = {1: ((1, 1), (60, 60), (60, 45)), 2: ((1, 2), (60, 30), (40, 30)), 3: ((2, 2), (30, 30), (30, 23)),
            4: ((2, 2), (30, 30), (30, 23)), 5: ((2, 3), (30, 20), (27, 20)), 6: ((2, 3), (30, 20), (27, 20)),
            7: ((3, 3), (20, 20), (20, 15)), 8: ((3, 3), (20, 20), (20, 15)), 9: ((3, 3), (20, 20), (20, 15))}
    for n, (grid, cell, tile) in fill.items():
        trailing = n < grid[0] * grid[1]
        c.append(Case(f"{n} equal sources at 60x30", "grid fill", [S] * n, (60, 30), grid, cell, _tiles(grid[0], cell, tile, range(n)),
                      canvas=_empty_trailing_cells if trailing else _tiles_lit_rest_black))
    # more than nine: the layout counts all of them, nine are placed, the cells behind the ninth stay empty.  80x30 is the
    # smallest terminal that gives four columns by three rows (cells of at least 20x10 terminal cells)
    for n in (10, 12):
        c.append(Case(f"{n} sources at 80x30", "grid fill", [S] * n, (80, 30), (4, 3), (20, 20), _tiles(4, (20, 20), (20, 15), range(9)),
                      canvas=_empty_trailing_cells))
    for name, dims, srcs in (("first", [None, S, S, S], (1, 2, 3)), ("in the middle", [S, None, S, S], (0, 2, 3)),
                             ("last", [S, S, S, None], (0, 1, 2))):
        c.append(Case(f"a client without video {name}", "grid fill", dims, (40, 20), (2, 2), (20, 20), _tiles(2, (20, 20), (20, 15), srcs),
                      canvas=_empty_trailing_cells))
    c.append(Case(ALL_NONE, "cell sizes", [None, None], (20, 4), (0, 0), (0, 0), [], canvas=_all_black))
    # ---- cell remainders ------------------------------------------------------------------------------------------
    c.append(Case("three columns at width 62", "cell remainders", [S] * 3, (62, 10), (3, 1), (20, 20), _tiles(3, (20, 20), (20, 15), range(3)),
                  canvas=_remainder))
    c.append(Case("3x3 on a 62x62 canvas", "cell remainders", [S] * 9, (62, 31), (3, 3), (20, 20), _tiles(3, (20, 20), (20, 15), range(9)),
                  canvas=_remainder))
    # ---- tiles ----------------------------------------------------------------------------------------------------
    one = (20, 10)  # one cell of 20x20 pixels
    c.append(Case("a wide source", "tiles", [(16, 2)], one, (1, 1), (20, 20), [(20, 3, 0, 8, 0)], canvas=_margins(True)))
    c.append(Case("a tall source", "tiles", [(2, 16)], one, (1, 1), (20, 20), [(3, 20, 8, 0, 0)], canvas=_margins(False)))
    c.append(Case("a source of the cell's aspect", "tiles", [(5, 5)], one, (1, 1), (20, 20), [(20, 20, 0, 0, 0)], canvas=_tile_is_cell))
    c.append(Case("a tile one pixel wide", "tiles", [(1, 20)], one, (1, 1), (20, 20), [(1, 20, 9, 0, 0)], canvas=_odd_margins))
    c.append(Case("a tile one pixel high", "tiles", [(20, 1)], one, (1, 1), (20, 20), [(20, 1, 0, 9, 0)], canvas=_odd_margins))
    c.append(Case("tile_w rounds to 0 in the middle of the grid", "tiles", [S, (1, 50), S, S], (40, 20), (2, 2), (20, 20),
                  [(20, 15, 0, 2, 0), None, (20, 15, 0, 22, 2), (20, 15, 20, 22, 3)], canvas=_hole_in_the_middle))
    # (130 columns: wider than the emulator's smallest rows geometry holds, which must say so)
    c.append(Case("a small tile in a row of 130 cells", "tiles", [S], (130, 2), (1, 1), (130, 4), [(5, 4, 62, 0, 0)], canvas=_margins(False)))
    c.append(Case("odd margins", "tiles", [(7, 5)], (21, 10), (1, 1), (21, 20), [(21, 15, 0, 2, 0)], canvas=_odd_margins))
    # ---- sources --------------------------------------------------------------------------------------------------
    c.append(Case("a 1x1 source", "sources", [(1, 1)], one, (1, 1), (20, 20), [(20, 20, 0, 0, 0)], canvas=_one_pixel_sources))
    c.append(Case("2x1 and 1x2 sources", "sources", [(2, 1), (1, 2)], (20, 20), (1, 2), (20, 20), [(20, 10, 0, 5, 0), (10, 20, 5, 20, 1)],
                  canvas=_tiles_lit_rest_black))
    c.append(Case("an upscaled source", "sources", [(3, 2)], one, (1, 1), (20, 20), [(20, 13, 0, 3, 0)], canvas=_upscaled))
    c.append(Case("a downscaled 33x77 source", "sources", [(33, 77)], one, (1, 1), (20, 20), [(9, 20, 5, 0, 0)], canvas=_tiles_lit_rest_black))
    c.append(Case("sources of different sizes", "sources", [S, (33, 77), (1, 1), (16, 2)], (40, 20), (2, 2), (20, 20),
                  [(20, 15, 0, 2, 0), (9, 20, 25, 0, 1), (20, 20, 0, 20, 2), (20, 3, 20, 28, 3)], canvas=_one_pixel_sources))
    # ---- cell sizes -----------------------------------------------------------------------------------------------
    c.append(Case(ONE_PIXEL_CELL_H, "cell sizes", [S] * 9, (20, 5), (1, 9), (20, 1), _tiles(1, (20, 1), (1, 1), range(9)), canvas=_remainder))
    c.append(Case("cell_h == 2: nine sources at 20x9", "cell sizes", [S] * 9, (20, 9), (1, 9), (20, 2), _tiles(1, (20, 2), (3, 2), range(9)),
                  canvas=_tiles_lit_rest_black))
    c.append(Case(ONE_PIXEL_CELLS, "cell sizes", [S] * 9, (1, 5), (1, 9), (1, 1), _tiles(1, (1, 1), (1, 1), range(9)), canvas=_remainder))
    c.append(Case(ZERO_CELL, "cell sizes", [S] * 9, (20, 4), (1, 9), (20, 0), [None] * 9, canvas=_all_black))
    assert len({k.name for k in c}) == len(c)
    return c


def wire_expect(frame, width, height):
    """-> (crc, 24-byte header, packet crc) of a frame sent as it is: orc.crc32c and zhuf_ref.packet_header over the oracle's bytes"""
    import zhuf_ref
    crc = orc.crc32c(frame)
    hdr = zhuf_ref.packet_header(width, height, len(frame), 0, crc, 0)
    pkt = orc.crc32c(hdr + frame)
    assert (hdr, pkt) == orc.ascii_frame_packet(frame, width, height), "the two references agree"
    return crc, hdr, pkt


FAMILIES = ("grid fill", "cell remainders", "tiles", "sources", "cell sizes")
