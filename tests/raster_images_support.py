"""Cells straight from frame descriptors (asciichat_raster_images_set and the entries behind it): the case table the emulated and
the GPU tests share, a face atlas in which every glyph has coverage, and the expectation -- the existing chain on the CPU, the
oracle's text for what a descriptor samples parsed and painted by the restatement (raster_ref.render).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emubuild
import orc
import raster_ref as RR
import raster_support as RS
from achip_ctypes import MODE_CAPS, MODE_NAMES, Frame

FILL = RS.FILL
NO_GLYPH = 0xFFFF
MONO, TRUE_FG, FG256, FG16, TRUE_BG, HB_TRUE, HB_256, HB_16, HB_MONO = range(9)
HALF_BLOCK = (HB_TRUE, HB_256, HB_16, HB_MONO)
FLIP_X, FLIP_Y, TINT, FG_OVERRIDE = 1, 2, 4, 64
PALETTE_MIXED = ".:▒█"  # one-byte and multi-byte glyphs that all draw: Y < 43 '.', < 128 ':', < 213 U+2592, else U+2588


# ---- the face ---------------------------------------------------------------------------------------------------------------
def _build_atlases():
    """cell 6x11, printable ASCII with the space, the upper half block and the four shades; noise coverage without a zero, so
    both colours of every cell that draws reach its pixels; some glyphs a pixel over their cell"""
    rng = np.random.default_rng(21)
    spec = []
    for cp in list(range(32, 127)) + [0x2580, 0x2591, 0x2592, 0x2593, 0x2588]:
        left, top = -(cp % 3 == 0), 8 + (cp % 5 == 0)
        w, rows = 6 + (cp % 3 == 0) + (cp % 7 == 0), 9 + (cp % 4)
        spec.append((cp, left, top, w, rows, 0, rng.integers(1, 256, size=w * rows, dtype=np.uint8)))
    face = RS._atlas(6, 11, 8, spec, 22, default_fg=0xC8C9CA, default_bg=0x101112, indexed=RR.INDEXED_XTERM)
    a = {"face": face, "face_flat": face.replace(indexed=RR.INDEXED_FLAT, flat_fg=0x0A141E, flat_bg=0xF0E6DC)}
    lacking = face.replace()
    lacking.glyphs = [g for g in face.glyphs if g.codepoint != ord("o")]
    a["face_without_o"] = lacking
    a["matrix"] = RS.ATLASES["matrix"]
    return a


ATLASES = _build_atlases()


# ---- sources and cases ------------------------------------------------------------------------------------------------------
class Src:
    """one frame: an image, how its descriptor is made (("convert", width, height, wants_padding, use_aspect) through
    achip_frame_setup, or ("identity",)), an explicit row stride, and the display path's ops"""

    def __init__(self, img, setup, stride=0, flip=(False, False), flt=0, rainbow=None):
        self.img = np.ascontiguousarray(img, dtype=np.uint8)
        self.setup, self.stride, self.flip, self.flt, self.rainbow = setup, stride, flip, flt, rainbow
        h, w = self.img.shape[:2]
        row = stride or 3 * w
        self.buf = np.full((h - 1) * row + 3 * w + 16, 0x5A, dtype=np.uint8)  # (row padding and the tail: never a sample)
        for y in range(h):
            self.buf[y * row:y * row + 3 * w] = self.img[y].reshape(-1)


class Case:
    def __init__(self, mode, frames, cols, rows, palette=orc.PALETTE_STANDARD, atlas="face", max_frames=None, n=None, status=None,
                 base_off=0, pitch_extra=0):
        self.mode, self.frames, self.cols, self.rows, self.palette, self.atlas = mode, list(frames), cols, rows, palette, atlas
        self.max_frames = len(self.frames) if max_frames is None else max_frames
        self.n = len(self.frames) if n is None else n  # frames run, of those set
        self.status, self.base_off, self.pitch_extra = status, base_off, pitch_extra

    @property
    def font(self):
        return ATLASES[self.atlas]


def noise(w, h, seed=1):
    return orc.frame_hash_noise(w, h, seed)


def _conv(w, h, cols, rows, pad=False, aspect=False, seed=1, **kw):
    return Src(noise(w, h, seed), ("convert", cols, rows, pad, aspect), **kw)


def _ident(img, **kw):
    return Src(np.asarray(img, dtype=np.uint8), ("identity",), **kw)


def _transparent_source():
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    img[0:2, 4:8] = noise(4, 2, 5)
    img[0:2, 4:8] |= 1  # (no sample of the coloured part is black)
    return img


def _run_head_source():
    # cells 0-2 quantise like black and the run's first cell IS black: all three are spaces; cells 4-7 quantise like black too,
    # but their run begins with (1, 1, 1): all four draw, the black ones included
    row = [(0, 0, 0), (1, 1, 1), (0, 0, 0), (200, 10, 10), (1, 1, 1), (0, 0, 0), (0, 0, 0), (2, 2, 2)]
    return np.array([row, row], dtype=np.uint8)


def _shade_source():
    # l = 255 v >> 8: 15 | 16, 63 | 64, 127 | 128, 191 | 192 on the upper half; the lower half dark, but for one cell that is
    # dark above and bright below (drawn, with the first shade)
    top = [(v, v, v) for v in (16, 17, 64, 65, 128, 129, 192, 193, 3)]
    bottom = [(0, 0, 0)] * 8 + [(90, 90, 90)]
    return np.array([top, bottom], dtype=np.uint8)


def _pen_source():
    # PALETTE_MIXED in TRUE_FG: A, B one-byte cells (dark), M a multi-byte cell (bright).  A M A A: the two A behind M equal the
    # A in front of it, emit nothing and show M's colour; B differs and sets its own; the second row begins with B again (equal to
    # the last one-byte cell, with an M in between) and so do its pad cells
    A, B, M, N = (10, 20, 30), (30, 20, 10), (200, 210, 220), (250, 240, 230)
    return np.array([[A, M, A, A, B, M], [B, B, N, A, A, M]], dtype=np.uint8)


def _batch():
    out = []
    for i in range(40):
        w, h = (48, 16) if i % 3 == 0 else (16, 48) if i % 3 == 1 else (33 + i, 7 + i % 5)
        cols, rows = (20, 6) if i % 4 else (23, 7)  # (every fourth frame is larger than the 20 x 6 grid)
        out.append(_conv(w, h, cols, rows, pad=i % 2 == 0, aspect=i % 2 == 0, seed=30 + i, flip=(i % 5 == 0, i % 7 == 0)))
    return out


def cases():
    c = {}
    for m in range(9):
        c[f"{MODE_NAMES[m]} 48x16 -> 16x4"] = Case(m, [_conv(48, 16, 16, 4)], 16, 4)
    for m in (TRUE_FG, FG256, HB_TRUE):
        c[f"{MODE_NAMES[m]} pad_left 8"] = Case(m, [_conv(16, 48, 20, 6, True, True)], 20, 6)
    for m in (TRUE_FG, HB_256):
        c[f"{MODE_NAMES[m]} pad_top"] = Case(m, [_conv(64, 8, 20, 6, True, True, seed=2)], 20, 6)
    for m in (HB_TRUE, HB_256, HB_16):
        c[f"{MODE_NAMES[m]} transparent run first"] = Case(m, [Src(_transparent_source(), ("convert", 8, 4, False, False))], 8, 4)
        c[f"{MODE_NAMES[m]} transparent run behind a coloured one"] = Case(
            m, [Src(_transparent_source(), ("convert", 8, 4, False, False), flip=(True, False))], 8, 4)
    for m in (HB_256, HB_16):
        c[f"{MODE_NAMES[m]} the run's first cell decides"] = Case(m, [_ident(_run_head_source())], 8, 1)
    for m in (HB_TRUE, HB_MONO):
        c[f"{MODE_NAMES[m]} odd height"] = Case(m, [_ident(noise(8, 5, 3))], 8, 3)
    c["hb_mono shade steps"] = Case(HB_MONO, [_ident(_shade_source())], 9, 1)
    c["true_fg blocks palette"] = Case(TRUE_FG, [_conv(48, 16, 16, 4)], 16, 4, palette=orc.PALETTE_BLOCKS)
    c["mono blocks palette"] = Case(MONO, [_conv(48, 16, 16, 4)], 16, 4, palette=orc.PALETTE_BLOCKS)
    c["true_fg one-character palette"] = Case(TRUE_FG, [_conv(48, 16, 16, 4)], 16, 4, palette="#")
    c["true_fg mixed palette on noise"] = Case(TRUE_FG, [_conv(16, 48, 20, 6, True, True)], 20, 6, palette=PALETTE_MIXED)
    pen = _ident(_pen_source())
    c["true_fg mixed palette: a pen outlives its cell"] = Case(TRUE_FG, [pen], 6, 2, palette=PALETTE_MIXED)
    c["true_fg a glyph the face lacks"] = Case(TRUE_FG, [_conv(48, 16, 16, 4)], 16, 4, atlas="face_without_o")
    c["mono matrix map with padding"] = Case(MONO, [_conv(16, 48, 20, 6, True, True)], 20, 6, atlas="matrix")
    for m in (FG256, FG16, HB_256):
        c[f"{MODE_NAMES[m]} flat indexed colours"] = Case(m, [_conv(48, 16, 16, 4)], 16, 4, atlas="face_flat")
    c["true_fg both flips"] = Case(TRUE_FG, [_conv(48, 16, 16, 4, flip=(True, True))], 16, 4)
    c["hb_true tint"] = Case(HB_TRUE, [_conv(48, 16, 16, 4, flt=3)], 16, 4)
    c["256_fg tint on white"] = Case(FG256, [_conv(48, 16, 16, 4, flt=1)], 16, 4)
    c["true_fg override with padding"] = Case(TRUE_FG, [_conv(16, 48, 20, 6, True, True, rainbow=1.3)], 20, 6)
    c["true_bg override"] = Case(TRUE_BG, [_conv(48, 16, 16, 4, rainbow=0.4)], 16, 4)
    c["hb_true override"] = Case(HB_TRUE, [Src(_transparent_source(), ("convert", 8, 4, False, False), rainbow=2.05)], 8, 4)
    c["true_fg row stride 160"] = Case(TRUE_FG, [_conv(48, 16, 16, 4, stride=160)], 16, 4)
    c["hb_16 row stride 160"] = Case(HB_16, [_conv(48, 16, 16, 4, stride=160, flip=(True, True))], 16, 4)
    for m in (TRUE_FG, HB_TRUE):
        c[f"{MODE_NAMES[m]} 1x1 source"] = Case(m, [Src(np.array([[[90, 160, 230]]]), ("convert", 5, 3, False, False))], 5, 3)
    c["true_fg out_w 1"] = Case(TRUE_FG, [_conv(9, 12, 1, 4)], 3, 4)
    c["true_fg grid larger than the frame"] = Case(TRUE_FG, [_conv(48, 16, 16, 4)], 20, 7, base_off=4, pitch_extra=20)
    for (cols, rows), st in (((15, 4), 8), ((16, 3), 16), ((8, 2), 24)):
        c[f"true_fg 16x4 frame into {cols}x{rows}"] = Case(TRUE_FG, [_conv(48, 16, 16, 4)], cols, rows, status=[st])
    c["hb_256 16x4 frame into 8x2"] = Case(HB_256, [_conv(48, 16, 16, 4)], 8, 2, status=[24])
    c["true_fg frame behind the grid's rows"] = Case(TRUE_FG, [_conv(64, 8, 20, 6, True, True, seed=2)], 8, 2, status=[16])
    c["true_fg 300x2: two workgroups, two tiles"] = Case(TRUE_FG, [_ident(noise(300, 2, 4))], 300, 2, base_off=12)
    c["mono 300x2"] = Case(MONO, [_ident(noise(300, 2, 4))], 300, 2)
    c["batch of 40 in a handle of 64"] = Case(TRUE_FG, _batch(), 20, 6, max_frames=64)
    c["33 of 40 frames set"] = Case(HB_256, _batch(), 20, 6, max_frames=64, n=33)
    return c


# ---- descriptors --------------------------------------------------------------------------------------------------------------
def descriptor(lib, cls, mode, src, address):
    """the achip_frame_t of a source whose buffer lives at `address`, built by the host helpers of `lib`"""
    f = cls()
    h, w = src.img.shape[:2]
    if src.setup[0] == "convert":
        _, width, height, pad, aspect = src.setup
        assert lib.achip_frame_setup(C.byref(f), address, w, h, width, height, 2 if mode in HALF_BLOCK else 0, pad, aspect, False) == 0
    else:
        assert lib.achip_frame_identity(C.byref(f), address, w, h) == 0
    f.src_stride = src.stride
    assert lib.achip_frame_set_display_ops(C.byref(f), src.flip[0], src.flip[1], src.flt) == 0
    if src.rainbow is not None:
        assert lib.achip_frame_set_rainbow(C.byref(f), src.rainbow) == 0 and f.ops & FG_OVERRIDE
    return f


def descriptors(lib, cls, case, addresses):
    return [descriptor(lib, cls, case.mode, s, a) for s, a in zip(case.frames, addresses)]


def sampled(desc, src):
    """the descriptor's rule (achip_types.h) in Python integers over the source's buffer, then the colour filter"""
    w, h = int(desc.src_w), int(desc.src_h)
    stride = int(desc.src_stride) or 3 * w
    xs = np.array([min((x * int(desc.x_ratio)) >> 16, w - 1) for x in range(int(desc.out_w))], dtype=np.int64)
    ys = np.array([min((y * int(desc.y_ratio)) >> 16, h - 1) for y in range(int(desc.out_h))], dtype=np.int64)
    if desc.ops & FLIP_X:
        xs = w - 1 - xs
    if desc.ops & FLIP_Y:
        ys = h - 1 - ys
    idx = ys[:, None] * stride + 3 * xs[None, :]
    img = np.ascontiguousarray(np.stack([src.buf[idx], src.buf[idx + 1], src.buf[idx + 2]], axis=-1), dtype=np.uint8)
    return orc.color_filter(img, src.flt) if src.flt else img


def text(mode, palette, desc, src):
    """the bytes the reference emits for what the descriptor samples: what Plan.render writes for it"""
    img = sampled(desc, src)
    s = orc.print_truecolor_bg(img, palette) if mode == TRUE_BG else orc.print_with_caps(img, *MODE_CAPS[mode], palette)
    assert s, "the oracle emitted nothing"
    s = orc.pad_height(orc.pad_width(s, int(desc.pad_left)), int(desc.pad_top))
    return orc.rainbow_replace(s, src.rainbow) if src.rainbow is not None else s


def slot_of(font, cp):
    """the parse kernel's lookup"""
    if cp in (0, 0x20):
        return NO_GLYPH
    if font.matrix_map:
        cp = RR.matrix_char_map(cp)
    for k, g in enumerate(font.glyphs):
        if g.codepoint == cp:
            return k
    return NO_GLYPH


_expected = {}


def expected(name, case, lib=None, cls=Frame):
    """[(image, status, cells as uint32[rows * cols][3])] of the frames a case runs, by the existing chain on the CPU; once"""
    if name not in _expected:
        if lib is None:
            import emu
            lib = emu.lib()
        out = []
        descs = descriptors(lib, cls, case, [s.buf.ctypes.data for s in case.frames])
        for d, s in list(zip(descs, case.frames))[:case.n]:
            frame = text(case.mode, case.palette, d, s)
            cells, st = RR.parse(frame, case.cols, case.rows, case.font)
            img = RR.rasterise(cells, case.cols, case.rows, case.font)
            img.setflags(write=False)
            flat = np.array([[slot_of(case.font, cp), fg, bg] for row in cells for cp, fg, bg in row], dtype=np.uint32)
            out.append((img, st, flat))
        _expected[name] = out
    return _expected[name]


# ---- running a case -------------------------------------------------------------------------------------------------------------
def pixel_buffer(case, base=None):
    """raster_support's guard-filled buffer, with room for every frame SET: those not run must stay untouched"""
    return RS.pixel_buffer(case, base)


def check(name, case, exp, pixels, start, pitch, status, cells=None):
    f = case.font
    H, W = case.rows * f.cell_h, case.cols * f.cell_w
    nb = 4 * W * H
    assert len(exp) == case.n
    assert (pixels[:start] == FILL).all(), f"{name}: a store in front of the first image"
    for i, (img, st, flat) in enumerate(exp):
        if cells is not None:
            got_cells = cells[i * case.rows * case.cols:(i + 1) * case.rows * case.cols]
            assert np.array_equal(got_cells, flat), f"{name} frame {i}: first cells that differ {np.argwhere(got_cells != flat)[:6].tolist()}"
        got = pixels[start + i * pitch:start + i * pitch + nb].reshape(H, W, 4)
        assert np.array_equal(got, img), f"{name} frame {i}: first differences (y, x, channel) {np.argwhere(got != img)[:6].tolist()}"
        assert (pixels[start + i * pitch + nb:start + (i + 1) * pitch] == FILL).all(), f"{name} frame {i}: a store beyond the image"
        assert int(status[i]) == st, f"{name} frame {i}: status {int(status[i])}, the parser's {st}"
        assert st & ~(RR.OVERFLOW_COLS | RR.OVERFLOW_ROWS) == 0
        if case.status is not None:
            assert st == case.status[i], f"{name} frame {i}: the parser reports {st}, the case expects {case.status[i]}"
    assert (pixels[start + case.n * pitch:] == FILL).all(), f"{name}: a store past the last image run"
    assert (np.asarray(status[case.n:]) == 0xABABABAB).all(), f"{name}: a status behind the frames run"


_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libraster_images_emu.so", "raster_images_emu_driver.cpp",
                                           ("raster_images_kernels.hpp", "raster_images.h", "achip_desc.h", "raster_kernels.hpp",
                                            "render_kernels.hpp", "raster.h", "asciichat_raster.h", "achip_types.h")))
        L.emu_raster_images.restype = C.c_int
        L.emu_raster_images.argtypes = [C.POINTER(RS.CFont), C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(Frame), C.c_int,
                                        C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.emu_raster_images_check.restype = C.c_int
        L.emu_raster_images_check.argtypes = [C.c_int, C.c_char_p, C.POINTER(Frame), C.c_int, C.c_int, C.POINTER(C.c_char_p)]
        L.emu_raster_images_cells_per_group.restype = C.c_int
        _emu = L
    return _emu


def emu_run(case):
    """-> (pixels, start, pitch, status, cells as uint32[n * rows * cols][3])"""
    import emu
    descs = descriptors(emu.lib(), Frame, case, [s.buf.ctypes.data for s in case.frames])
    arr = (Frame * len(descs))(*descs)
    pixels, start, pitch = pixel_buffer(case)
    status = np.full(len(case.frames), 0xABABABAB, dtype=np.uint32)
    cells = np.zeros((case.n * case.rows * case.cols, 3), dtype=np.uint32)
    font = RS.c_font(case.font)
    rc = emulator().emu_raster_images(C.byref(font), case.cols, case.rows, case.max_frames, case.mode, case.palette.encode("utf-8"), arr,
                                      len(descs), case.n, pixels.ctypes.data + start, pitch, status.ctypes.data, cells.ctypes.data)
    assert rc == 0, f"the font, the grid or the set was refused ({rc})"
    return pixels, start, pitch, status, cells
