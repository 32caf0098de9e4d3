"""Cells straight from grid composites (asciichat_raster_images_set_composites and the entries behind it): the case table the
emulated and the GPU tests share, built over the boundary families of composite_cases.py, and the expectation -- the oracle's
text for the case's canvas (composite_cases.Case.expected), parsed and painted by the restatement (raster_ref.parse and
raster_ref.rasterise) with the face atlas of raster_images_support.py.  A composite frame's descriptor is built as
test_gpu_composite.py builds it.  TESTS ONLY."""
import ctypes as C

import numpy as np

import composite_cases as CC
import emubuild
import orc
import raster_images_support as RI
import raster_ref as RR
import raster_support as RS
from achip_ctypes import MODE_CAPS, MODE_NAMES, MODE_TRUE_BG, Composite, Frame

FILL = RI.FILL
MONO, TRUE_FG, FG256, FG16, TRUE_BG, HB_TRUE, HB_256, HB_16, HB_MONO = range(9)
HALF_BLOCK = RI.HALF_BLOCK
STD = orc.PALETTE_STANDARD
BY_NAME = {k.name: k for k in CC.cases()}
NINE, HOLE = "9 equal sources at 60x30", "tile_w rounds to 0 in the middle of the grid"
NEAR_BLACK = (1, 1, 1)  # quantises like black in the 256- and the 16-colour modes, and is not black


def _crafted(name, dims, term, grid, cell, tiles, imgs, canvas):
    k = CC.Case(name, "crafted", dims, term, grid, cell, tiles, canvas=canvas)
    k._imgs = [np.ascontiguousarray(i, dtype=np.uint8) for i in imgs]
    return k


def _margin_tile():
    """"a tall source" (a tile 3 pixels wide at x = 8 of its 20-pixel cell, black margins on both sides) whose left source
    column is near-black: the tile's first cells belong to the run the black margin began"""
    img = orc.frame_hash_noise(2, 16, 61) | 0x40
    img[:, 0] = NEAR_BLACK
    return _crafted("near-black tile edge behind a black margin", [(2, 16)], (20, 10), (1, 1), (20, 20), [(3, 20, 8, 0, 0)], [img],
                    CC._margins(False))


def _edge_tile():
    """"a source of the cell's aspect" (the tile fills its cell from column 0) whose first source column is near-black and whose
    second is black: the row's first run begins with the near-black cell"""
    img = orc.frame_hash_noise(5, 5, 62) | 0x40
    img[:, 0] = NEAR_BLACK
    img[:, 1] = 0
    return _crafted("near-black tile edge at column 0", [(5, 5)], (20, 10), (1, 1), (20, 20), [(20, 20, 0, 0, 0)], [img],
                    CC._tiles_lit_rest_black)


def _bright_tile():
    """"a tall source" again, every pixel bright (Y >= 213: PALETTE_MIXED's multi-byte U+2588) between black margins (Y = 0: its
    one-byte '.'): the black cells behind the tile equal the black cells in front of it, emit no colour and show the tile's"""
    img = orc.frame_hash_noise(2, 16, 63) | 0xE0
    return _crafted("bright tile between black margins", [(2, 16)], (20, 10), (1, 1), (20, 20), [(3, 20, 8, 0, 0)], [img], CC._margins(False))


MARGIN_TILE, EDGE_TILE, BRIGHT_TILE = _margin_tile(), _edge_tile(), _bright_tile()
for _k in (MARGIN_TILE, EDGE_TILE, BRIGHT_TILE):
    BY_NAME[_k.name] = _k


class Comp:
    """one composite frame: a case of composite_cases.py (or a crafted one), display ops (flip_x, flip_y, filter) and a rainbow
    override as achip_frame_set_display_ops / achip_frame_set_rainbow take them"""

    def __init__(self, case, ops=None, rainbow=None):
        self.case = BY_NAME[case] if isinstance(case, str) else case
        self.ops, self.rainbow = ops, rainbow

    def text(self, mode, palette):
        """the oracle's frame for the canvas: flips and tints do not reach a composite frame, the override does"""
        k = self.case
        if palette == STD:
            s = k.expected(mode)
        else:  # Case.expected's own calls, with the palette
            tw, th = k.term
            if mode == MODE_TRUE_BG:
                s = orc.print_truecolor_bg(orc.resize_nn(k.canvas(), tw, th), palette)
            else:
                cl, rm = MODE_CAPS[mode]
                s = orc.convert_with_caps(k.canvas(), tw, k.frame_height(mode), cl, rm, True, True, False, palette=palette)
        return orc.rainbow_replace(s, self.rainbow) if self.rainbow is not None else s


def comp_frame(lib, cls, mode, item, comp_address):
    """test_gpu_composite.py's descriptor: no source of its own, the canvas's size, the composite's address"""
    tw, th = item.case.term
    f = cls()
    assert lib.achip_frame_setup(C.byref(f), None, tw, 2 * th, tw, item.case.frame_height(mode), MODE_CAPS.get(mode, (3, 0))[1], True, True,
                                 False) == 0
    f.comp = comp_address
    if item.ops:
        assert lib.achip_frame_set_display_ops(C.byref(f), *item.ops) == 0 and f.ops
    if item.rainbow is not None:
        assert lib.achip_frame_set_rainbow(C.byref(f), item.rainbow) == 0 and f.ops & RI.FG_OVERRIDE
    return f


def grid_of(lib, cls, mode, item):
    """the grid a frame's text fills: cols = pad_left + out_w, rows = pad_top + text rows, from its descriptor"""
    f = comp_frame(lib, cls, mode, item, 1) if isinstance(item, Comp) else RI.descriptor(lib, cls, mode, item, 1)
    t = f.out_h - (f.out_h >> 1) if mode in HALF_BLOCK else f.out_h
    return f.pad_left + f.out_w, f.pad_top + t


class Case:
    """RI.Case's fields (RI.check and RS.pixel_buffer read them); frames are Comp or RI.Src.  cols, rows None: the smallest grid
    that holds every frame's text, from the descriptors, and then the expected status is 0"""

    def __init__(self, mode, frames, cols=None, rows=None, palette=STD, atlas="face", max_frames=None, n=None, status=None, base_off=0,
                 pitch_extra=0):
        self.mode, self.frames, self.palette, self.atlas = mode, list(frames), palette, atlas
        self.cols, self.rows = cols, rows
        self.max_frames = len(self.frames) if max_frames is None else max_frames
        self.n = len(self.frames) if n is None else n
        self.status, self.base_off, self.pitch_extra = status, base_off, pitch_extra
        self.sized = cols is None

    def size(self, lib, cls=Frame):
        """(cls: the structure class lib's prototypes were declared with)"""
        if self.cols is None:
            self.cols, self.rows = (max(v) for v in zip(*[grid_of(lib, cls, self.mode, it) for it in self.frames]))
        return self

    @property
    def font(self):
        return RI.ATLASES[self.atlas]


COVERAGE = ["a client without video in the middle", CC.ALL_NONE, "three columns at width 62", "3x3 on a 62x62 canvas", "a wide source",
            "a small tile in a row of 130 cells", "a 1x1 source", "sources of different sizes", CC.ONE_PIXEL_CELLS, CC.ZERO_CELL]
FLAGGED = "5 equal sources at 60x30"


def _mixed_batch(mode):
    plain = RI.Src(RI.noise(48, 16, 71), ("convert", 60, 30, False, False), flip=(True, False), flt=3)
    return [plain, Comp(NINE), Comp("sources of different sizes"), Comp(NINE), Comp(HOLE), plain]


def cases():
    c = {}
    for m in range(9):  # 60 x 30 = 1800 cells: 8 workgroups stage the same descriptor, the last with 248 idle lanes
        c[f"{MODE_NAMES[m]} {NINE}"] = Case(m, [Comp(NINE)])
        c[f"{MODE_NAMES[m]} {HOLE}"] = Case(m, [Comp(HOLE)])
    for i, name in enumerate(COVERAGE):  # every family, two modes each, one of them a half-block mode
        for m in ((TRUE_FG, HB_256), (FG256, HB_TRUE), (TRUE_BG, HB_16), (MONO, HB_MONO), (FG16, HB_TRUE))[i % 5]:
            c[f"{MODE_NAMES[m]} {name}"] = Case(m, [Comp(name)])
    # the walks across tile edges
    c["true_fg mixed palette over nine tiles"] = Case(TRUE_FG, [Comp(NINE)], palette=RI.PALETTE_MIXED)
    c["true_fg mixed palette over margins"] = Case(TRUE_FG, [Comp("sources of different sizes")], palette=RI.PALETTE_MIXED)
    c[f"true_fg mixed palette, {BRIGHT_TILE.name}"] = Case(TRUE_FG, [Comp(BRIGHT_TILE)], palette=RI.PALETTE_MIXED)
    for m in (HB_256, HB_16):
        c[f"{MODE_NAMES[m]} {MARGIN_TILE.name}"] = Case(m, [Comp(MARGIN_TILE)])
        c[f"{MODE_NAMES[m]} {EDGE_TILE.name}"] = Case(m, [Comp(EDGE_TILE)])
    # the flags: flips and a tint change nothing, the override acts
    for m in (TRUE_FG, HB_TRUE, FG256):
        c[f"{MODE_NAMES[m]} flips and a tint on a composite"] = Case(m, [Comp(FLAGGED, ops=(True, True, 3))])
    for m, t in ((TRUE_FG, 1.3), (TRUE_BG, 0.4), (HB_TRUE, 2.05)):
        c[f"{MODE_NAMES[m]} override on a composite"] = Case(m, [Comp(FLAGGED, rainbow=t)])
    # a grid too small: 60 x 30 text into 59 x 30, 60 x 29, 31 x 7
    for (cols, rows), st in (((59, 30), 8), ((60, 29), 16), ((31, 7), 24)):
        c[f"true_fg nine tiles into {cols}x{rows}"] = Case(TRUE_FG, [Comp(NINE)], cols, rows, status=[st])
    # (the half-block frame is 60 x 30 text rows under 15 rows of padding)
    c["hb_256 nine tiles into 31x20"] = Case(HB_256, [Comp(NINE)], 31, 20, status=[24])
    c["hb_256 nine tiles behind the rows of 31x7"] = Case(HB_256, [Comp(NINE)], 31, 7, status=[16])
    # plain and composite frames in one set, more room in the handle than frames set, fewer run than set
    for m in (TRUE_FG, HB_256):
        c[f"{MODE_NAMES[m]} mixed batch: 4 of 6 set, handle of 8"] = Case(m, _mixed_batch(m), max_frames=8, n=4, base_off=4, pitch_extra=20)
    return c


PLAIN_ONLY = "plain frames only"


def plain_only_case(mode=TRUE_FG):
    """a set without a composite frame: what either entry must treat alike"""
    return Case(mode, [RI.Src(RI.noise(48, 16, 72), ("convert", 20, 6, True, True)), RI.Src(RI.noise(16, 48, 73), ("convert", 20, 6, True, True))],
                20, 6)


# ---- descriptors and the expectation ------------------------------------------------------------------------------------------
def descriptors(lib, cls, case, comp_address, src_address):
    """comp_address(composite case) / src_address(RI.Src) -> where the frame's composite descriptor / source buffer lives"""
    return [comp_frame(lib, cls, case.mode, it, comp_address(it.case)) if isinstance(it, Comp)
            else RI.descriptor(lib, cls, case.mode, it, src_address(it)) for it in case.frames]


_expected = {}


def expected(name, case, lib=None, cls=Frame):
    """[(image, status, cells as uint32[rows * cols][3])] of the frames a case runs: the oracle's text through the restatement;
    computed once and left unchanged"""
    if name not in _expected:
        if lib is None:
            import emu
            lib = emu.lib()
        case.size(lib, cls)
        out = []
        for it in case.frames[:case.n]:
            if isinstance(it, Comp):
                frame = it.text(case.mode, case.palette)
            else:
                frame = RI.text(case.mode, case.palette, RI.descriptor(lib, cls, case.mode, it, it.buf.ctypes.data), it)
            cells, st = RR.parse(frame, case.cols, case.rows, case.font)
            if case.sized:
                assert st == 0, (name, st, "a grid made from the descriptor holds the oracle's text")
            img = RR.rasterise(cells, case.cols, case.rows, case.font)
            img.setflags(write=False)
            flat = np.array([[RI.slot_of(case.font, cp), fg, bg] for row in cells for cp, fg, bg in row], dtype=np.uint32)
            flat.setflags(write=False)
            out.append((img, st, flat))
        _expected[name] = out
    return _expected[name]


def pixel_buffer(case, base=None):
    return RS.pixel_buffer(case, base)


check = RI.check


# ---- the emulator ---------------------------------------------------------------------------------------------------------------
_emu = None
_host_comps = {}


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libraster_composites_emu.so", "raster_composites_emu_driver.cpp",
                                           ("raster_images_kernels.hpp", "raster_images.h", "achip_desc.h", "raster_kernels.hpp",
                                            "render_kernels.hpp", "raster.h", "asciichat_raster.h", "achip_types.h")))
        L.emu_raster_composites.restype = C.c_int
        L.emu_raster_composites.argtypes = [C.POINTER(RS.CFont), C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(Frame), C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.emu_raster_composites_check.restype = C.c_int
        L.emu_raster_composites_check.argtypes = [C.c_int, C.c_char_p, C.POINTER(Frame), C.c_int, C.c_int, C.POINTER(C.c_char_p),
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.emu_raster_composites_cells_per_group.restype = C.c_int
        L.emu_raster_composites_lds_bytes.restype = C.c_int
        _emu = L
    return _emu


def host_comp(k):
    """the case's descriptor over host memory (premise asserted), made once and kept alive"""
    import emu
    if k.name not in _host_comps:
        _host_comps[k.name] = k.host_descriptor(emu.lib())
    return _host_comps[k.name]


def emu_descriptors(case):
    import emu
    case.size(emu.lib())
    return descriptors(emu.lib(), Frame, case, lambda k: C.addressof(host_comp(k)), lambda s: s.buf.ctypes.data)


def emu_run(case, entry=0, force_comp=False, descs=None):
    """-> (pixels, start, pitch, status, cells as uint32[n * rows * cols][3], 1 when the form with the staged sampler ran)"""
    descs = emu_descriptors(case) if descs is None else descs
    arr = (Frame * len(descs))(*descs)
    pixels, start, pitch = pixel_buffer(case)
    status = np.full(len(case.frames), 0xABABABAB, dtype=np.uint32)
    cells = np.zeros((case.n * case.rows * case.cols, 3), dtype=np.uint32)
    font = RS.c_font(case.font)
    form = C.c_int(-1)
    rc = emulator().emu_raster_composites(C.byref(font), case.cols, case.rows, case.max_frames, case.mode, case.palette.encode("utf-8"), arr,
                                          len(descs), case.n, entry, int(force_comp), pixels.ctypes.data + start, pitch, status.ctypes.data,
                                          cells.ctypes.data, C.byref(form))
    assert rc == 0, f"the font, the grid or the set was refused ({rc})"
    return pixels, start, pitch, status, cells, form.value
