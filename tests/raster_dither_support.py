"""Cells straight from frame descriptors in the Floyd-Steinberg mode (asciichat_raster_images_set_dithered): the case table the
emulated and the GPU tests share and the expectation -- the oracle's dithered text (orc.print_16_dithered) for what a descriptor
samples, padded, then parsed and painted by the restatement (raster_ref.parse and raster_ref.rasterise) with the face atlas of
raster_images_support.py.  A frame is a raster_images_support.Src or a raster_composites_support.Comp with a `style`; for a
composite the sampled image is the composite support's (the oracle's canvas at the terminal's size).  The hand-built sources
that aim at the diffusion's arithmetic are checked here against a walk of that arithmetic in Python integers, itself held to the
oracle's text.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emubuild
import orc
import raster_composites_support as RC
import raster_images_support as RI
import raster_ref as RR
import raster_support as RS
from achip_ctypes import MODE_16_DITHER_BG, Frame

MODE = MODE_16_DITHER_BG
FILL = RI.FILL
BG, FG, RAMP = 0, 16, 48  # a frame's style as its ops carry it: none, DITHER_FG, DITHER_FG | DITHER_RAMP
STYLES = {"background": BG, "foreground": FG, "foreground with the ramp glyph": RAMP}
STD = orc.PALETTE_STANDARD
COMP_SMALL = "a source of the cell's aspect"  # the composite support's smallest grid with a picture in it: 20 x 10
ANSI16 = [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128), (192, 192, 192),
          (128, 128, 128), (255, 0, 0), (0, 255, 0), (255, 255, 0), (0, 0, 255), (255, 0, 255), (0, 255, 255), (255, 255, 255)]


def styled(item, style):
    item.style = style
    return item


def _conv(w, h, cols, rows, pad=False, aspect=False, seed=1, style=BG, **kw):
    return styled(RI.Src(RI.noise(w, h, seed), ("convert", cols, rows, pad, aspect), **kw), style)


def _ident(img, style=BG, **kw):
    return styled(RI.Src(np.asarray(img, dtype=np.uint8), ("identity",), **kw), style)


def _comp(name, style=BG, **kw):
    return styled(RC.Comp(name, **kw), style)


class Case:
    """RI.Case's fields (RI.check and RS.pixel_buffer read them); cols, rows None: the smallest grid that holds every frame's
    text, from the descriptors"""

    def __init__(self, frames, cols=None, rows=None, palette=STD, atlas="face", max_frames=None, n=None, status=None, base_off=0,
                 pitch_extra=0):
        self.mode, self.frames, self.palette, self.atlas = MODE, list(frames), palette, atlas
        self.cols, self.rows = cols, rows
        self.max_frames = len(self.frames) if max_frames is None else max_frames
        self.n = len(self.frames) if n is None else n
        self.status, self.base_off, self.pitch_extra = status, base_off, pitch_extra

    def size(self, lib, cls=Frame):
        if self.cols is None:
            ds = [descriptor(lib, cls, it, 1) for it in self.frames]
            self.cols, self.rows = max(d.pad_left + d.out_w for d in ds), max(d.pad_top + d.out_h for d in ds)
        return self

    @property
    def font(self):
        return RI.ATLASES[self.atlas]


# ---- the hand-built sources ---------------------------------------------------------------------------------------------------
def _flat(v, w=12, h=6):
    return np.full((h, w, 3), v, dtype=np.uint8)


def _rows(first, rest, tail, w=12):
    """a row of `first`, two of `rest` (where the running value leaves the bytes), three of `tail` (where the index of a sample
    shows which error travelled: walk() with the clamped error gives other indices, check_arithmetic_cases)"""
    img = np.full((6, w, 3), tail, dtype=np.uint8)
    img[0], img[1:3] = first, rest
    return img


ARITHMETIC = {
    "flat 250: negative errors, truncation is not floor": _flat(250),
    "flat 120: errors of both signs": _flat(120),
    "150, 255, 255, then 150s: the running value leaves 255": _rows(150, 255, 150),
    "100, 0, 0, then 80s: the running value leaves 0": _rows(100, 0, 80),
}


def batch():
    """RI._batch()'s sizes, flips and paddings, the three styles in turn"""
    return [styled(s, (BG, FG, RAMP)[i % 3]) for i, s in enumerate(RI._batch())]


CAP = 16384  # the kernel's band: RASTER_DITHER_CAP samples (the emulated test holds this restatement to the kernel's own rule)


def band_rows(out_w):
    """text rows of a band: as many as CAP samples hold, whole sweeps of 64 where more than 64 fit"""
    fit = CAP // out_w
    return fit & ~63 if fit > 64 else fit


def seam_cases():
    """{name: Case} -- one per band seam of the kernel: a frame 129 wide has bands of 64 rows (whole sweeps: CAP / 129 = 127 rounds
    down to 64), one 300 wide has bands of CAP / 300 rows (a band is one sweep of fewer than 64)"""
    c = {}
    assert band_rows(129) == 64
    c["band seam behind 64 rows of 129: a second band of 2 rows"] = Case([_ident(RI.noise(129, 66, 8))], 129, 66)
    b = band_rows(300)
    assert 1 < b < 64 and b == CAP // 300
    c[f"band seam behind {b} rows of 300: a second band of 1 row"] = Case([_ident(RI.noise(300, b + 1, 9), style=FG)], 300, b + 1)
    return c


def cases():
    c = {}
    for name, st in STYLES.items():
        c[f"{name} 48x16 -> 16x4"] = Case([_conv(48, 16, 16, 4, style=st)], 16, 4)
    c["out_w 1"] = Case([_conv(9, 12, 1, 4)], 3, 4)
    c["out_w 2"] = Case([_conv(9, 12, 2, 4, style=FG)], 3, 4)
    c["out_h 1"] = Case([_conv(48, 16, 16, 1)], 16, 1)
    for w, h, what in ((5, 64, "one sweep that ends at the frame's end"), (5, 65, "a second sweep of one row"),
                       (3, 66, "a second sweep of two rows"), (4, 129, "a third sweep")):
        c[f"{w}x{h} rows: {what}"] = Case([_ident(RI.noise(w, h, 6))], w, h)
    c.update(seam_cases())
    for name, img in ARITHMETIC.items():
        c[name] = Case([_ident(img)], 12, 6)
    c["pad_left"] = Case([_conv(16, 48, 20, 6, True, True)], 20, 6)
    c["pad_top"] = Case([_conv(64, 8, 20, 6, True, True, seed=2, style=FG)], 20, 6)
    for (cols, rows), st in (((15, 4), 8), ((16, 3), 16), ((8, 2), 24)):
        c[f"16x4 frame into {cols}x{rows}"] = Case([_conv(48, 16, 16, 4)], cols, rows, status=[st])
    c["frame behind the grid's rows"] = Case([_conv(64, 8, 20, 6, True, True, seed=2)], 8, 2, status=[16])
    c["grid larger than the frame"] = Case([_conv(48, 16, 16, 4)], 20, 7, base_off=4, pitch_extra=20)
    c["both flips with a tint"] = Case([_conv(48, 16, 16, 4, flip=(True, True), flt=3)], 16, 4)
    c["override"] = Case([_conv(48, 16, 16, 4, rainbow=1.3)], 16, 4)
    c["row stride 160"] = Case([_conv(48, 16, 16, 4, stride=160, style=RAMP)], 16, 4)
    c["1x1 source"] = Case([styled(RI.Src(np.array([[[90, 160, 230]]]), ("convert", 5, 3, False, False)), BG)], 5, 3)
    c["blocks palette"] = Case([_conv(48, 16, 16, 4)], 16, 4, palette=orc.PALETTE_BLOCKS)
    c["a glyph the face lacks"] = Case([_conv(48, 16, 16, 4)], 16, 4, atlas="face_without_o")
    c["matrix map with padding"] = Case([_conv(16, 48, 20, 6, True, True, style=RAMP)], 20, 6, atlas="matrix")
    c["flat indexed colours"] = Case([_conv(48, 16, 16, 4)], 16, 4, atlas="face_flat")
    c["flat indexed colours, foreground"] = Case([_conv(48, 16, 16, 4, style=FG)], 16, 4, atlas="face_flat")
    c[BATCH] = Case(batch(), 20, 6, max_frames=64, n=33)
    c[COMPOSITE] = Case([_comp(COMP_SMALL)])
    c[MIXED] = Case([_conv(48, 16, 20, 10, style=RAMP, flip=(True, False)), _comp(COMP_SMALL, style=FG, ops=(True, True, 3)), _comp("a tall source")],
                    max_frames=4, base_off=4, pitch_extra=20)
    return c


BATCH = "33 of a batch of 40 in a handle of 64"
COMPOSITE = "a composite in the background form"
MIXED = "a plain and two composite frames of three styles"
MULTI = ("rows:", "band seam")  # the names of the cases with more than one sweep or band: run under other wave schedules too


# ---- descriptors --------------------------------------------------------------------------------------------------------------
def descriptor(lib, cls, item, address):
    """the achip_frame_t of a frame whose source buffer / composite descriptor lives at `address`, in the frame's style"""
    f = RC.comp_frame(lib, cls, MODE, item, address) if isinstance(item, RC.Comp) else RI.descriptor(lib, cls, MODE, item, address)
    assert lib.achip_frame_set_dither_style(C.byref(f), item.style == BG, item.style == RAMP) == 0
    assert f.ops & 48 == item.style
    return f


def descriptors(lib, cls, case, comp_address, src_address):
    return [descriptor(lib, cls, it, comp_address(it.case) if isinstance(it, RC.Comp) else src_address(it)) for it in case.frames]


# ---- the expectation ------------------------------------------------------------------------------------------------------------
def sampled(lib, cls, item):
    """(the out_h x out_w image the frame's descriptor samples, pad_left, pad_top)"""
    if isinstance(item, RC.Comp):  # flips and tints do not reach a composite frame
        k = item.case
        tw, th = k.term
        assert orc.aspect_ratio(tw, 2 * th, tw, th, False) == (tw, th), k.name
        d = descriptor(lib, cls, item, 1)
        assert (d.out_w, d.out_h, d.pad_left, d.pad_top) == (tw, th, 0, 0), k.name
        return orc.resize_nn(k.canvas(), tw, th), 0, 0
    d = descriptor(lib, cls, item, item.buf.ctypes.data)
    return RI.sampled(d, item), int(d.pad_left), int(d.pad_top)


def text(lib, cls, palette, item):
    img, pad_left, pad_top = sampled(lib, cls, item)
    s = orc.print_16_dithered(img, item.style == BG, palette, item.style == RAMP)
    assert s, "the oracle emitted nothing"
    if isinstance(item, RC.Comp) and item.style == BG and palette == STD:  # what the composite support expects of this mode
        assert s == item.case.expected(MODE)
    s = orc.pad_height(orc.pad_width(s, pad_left), pad_top)
    rainbow = getattr(item, "rainbow", None)
    if rainbow is not None:
        assert orc.rainbow_replace(s, rainbow) == s  # no truecolor SGR to replace
    return s


_expected = {}


def expected(name, case, lib=None, cls=Frame):
    """[(image, status, cells as uint32[rows * cols][3])] of the frames a case runs; computed once and left unchanged"""
    if name not in _expected:
        if lib is None:
            import emu
            lib = emu.lib()
        case.size(lib, cls)
        out = []
        for it in case.frames[:case.n]:
            cells, st = RR.parse(text(lib, cls, case.palette, it), case.cols, case.rows, case.font)
            img = RR.rasterise(cells, case.cols, case.rows, case.font)
            img.setflags(write=False)
            flat = np.array([[RI.slot_of(case.font, cp), fg, bg] for row in cells for cp, fg, bg in row], dtype=np.uint32)
            flat.setflags(write=False)
            out.append((img, st, flat))
        _expected[name] = out
    return _expected[name]


check = RI.check


def pixel_buffer(case, base=None):
    return RS.pixel_buffer(case, base)


# ---- the diffusion's arithmetic, walked in Python integers ----------------------------------------------------------------------
def _trunc(e, w):
    return -((-e * w) // 16) if e < 0 else (e * w) // 16


def walk(img, floor=False, clamped_error=False):
    """rgb_to_16color_dithered over an image -> (indices (H, W), facts): 7/3/5/1 sixteenths each truncated toward zero, what
    leaves the image dropped, the clamped value quantised, the error taken from the unclamped one.  floor / clamped_error: the
    two mistakes the hand-built sources are there to catch.  facts: what happened on the way."""
    h, w = img.shape[:2]
    err = np.zeros((h + 1, w + 2, 3), dtype=np.int64)
    idx = np.zeros((h, w), dtype=np.int64)
    facts = dict(negative=False, positive=False, inexact_negative=False, above=False, below=False)
    term = (lambda e, k: (e * k) // 16) if floor else _trunc
    for y in range(h):
        for x in range(w):
            v = [int(img[y, x, k]) + int(err[y, x + 1, k]) for k in range(3)]
            c = [min(255, max(0, a)) for a in v]
            facts["above"] |= any(a > 255 for a in v)
            facts["below"] |= any(a < 0 for a in v)
            i = int(orc.lib().orc_rgb_to_16(*c))
            idx[y, x] = i
            for k in range(3):
                e = (c[k] if clamped_error else v[k]) - ANSI16[i][k]
                facts["negative"] |= e < 0
                facts["positive"] |= e > 0
                facts["inexact_negative"] |= e < 0 and any((e * m) % 16 for m in (7, 3, 5, 1))
                if x + 1 < w:
                    err[y, x + 2, k] += term(e, 7)
                if y + 1 < h:
                    if x > 0:
                        err[y + 1, x, k] += term(e, 3)
                    err[y + 1, x + 1, k] += term(e, 5)
                    if x + 1 < w:
                        err[y + 1, x + 2, k] += term(e, 1)
    return idx, facts


def oracle_indices(img):
    """the colour index of every sample, read out of the oracle's foreground-only text"""
    h, w = img.shape[:2]
    cells, st = RR.parse(orc.print_16_dithered(img, False, STD), w, h, RI.ATLASES["face"])
    assert st == 0
    rgb = {r << 16 | g << 8 | b: i for i, (r, g, b) in enumerate(ANSI16)}
    return np.array([[rgb[fg] for _, fg, _ in row] for row in cells], dtype=np.int64)


def check_arithmetic_cases():
    """each hand-built source does what its name says, by the oracle's own arithmetic"""
    for name, img in ARITHMETIC.items():
        want = oracle_indices(img)
        got, facts = walk(img)
        assert np.array_equal(got, want), f"{name}: the walk is not the oracle's"
        if "truncation" in name:
            assert facts["inexact_negative"] and not np.array_equal(walk(img, floor=True)[0], want), name
        if "both signs" in name:
            assert facts["negative"] and facts["positive"], name
        if "leaves 255" in name:
            assert facts["above"] and not np.array_equal(walk(img, clamped_error=True)[0], want), name
        if "leaves 0" in name:
            assert facts["below"] and not np.array_equal(walk(img, clamped_error=True)[0], want), name


# ---- the emulator ---------------------------------------------------------------------------------------------------------------
_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libraster_dither_emu.so", "raster_dither_emu_driver.cpp",
                                           ("raster_dither_kernels.hpp", "raster_images_kernels.hpp", "raster_images.h", "achip_desc.h",
                                            "raster_kernels.hpp", "render_kernels.hpp", "raster.h", "asciichat_raster.h", "achip_types.h")))
        L.emu_raster_dither.restype = C.c_int
        L.emu_raster_dither.argtypes = [C.POINTER(RS.CFont), C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.emu_raster_dither_check.restype = C.c_int
        L.emu_raster_dither_check.argtypes = [C.c_char_p, C.POINTER(Frame), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]
        L.emu_raster_dither_band_rows.restype = C.c_int
        L.emu_raster_dither_band_rows.argtypes = [C.c_int]
        for f in (L.emu_raster_dither_cap, L.emu_raster_dither_max_w, L.emu_raster_dither_lds_bytes):
            f.restype = C.c_int
        _emu = L
    return _emu


def emu_descriptors(case):
    import emu
    case.size(emu.lib())
    return descriptors(emu.lib(), Frame, case, lambda k: C.addressof(RC.host_comp(k)), lambda s: s.buf.ctypes.data)


def emu_run(case, force_comp=False):
    """-> (pixels, start, pitch, status, cells as uint32[n * rows * cols][3])"""
    descs = emu_descriptors(case)
    arr = (Frame * len(descs))(*descs)
    pixels, start, pitch = pixel_buffer(case)
    status = np.full(len(case.frames), 0xABABABAB, dtype=np.uint32)
    cells = np.zeros((case.n * case.rows * case.cols, 3), dtype=np.uint32)
    font = RS.c_font(case.font)
    rc = emulator().emu_raster_dither(C.byref(font), case.cols, case.rows, case.max_frames, case.palette.encode("utf-8"), arr, len(descs),
                                      case.n, int(force_comp), pixels.ctypes.data + start, pitch, status.ctypes.data, cells.ctypes.data)
    assert rc == 0, f"the font, the grid or the set was refused ({rc})"
    return pixels, start, pitch, status, cells
