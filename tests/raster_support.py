"""Rasteriser test support: the kernels under the CPU emulator (tests/hipemu/raster_emu_driver.cpp), the procedural atlases,
guard-filled pixel buffers, and the case table the emulated and the GPU tests share.  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import emubuild
import raster_ref as RR

ROOT = emubuild.ROOT
LIB = os.path.join(ROOT, "ascii-chat_amd", "libasciichat_raster.so")
HIP_LIB = os.path.join(ROOT, "ascii-chat_amd", "libasciichat_hip.so")
FILL = 0xEE  # every pixel byte before the pass (box_support's guard-fill idiom)
LEN_OVERFLOW = 0xFFFFFFFF


class CGlyph(C.Structure):  # asciichat_raster_glyph_t
    _fields_ = [("codepoint", C.c_uint32), ("left", C.c_int16), ("top", C.c_int16), ("width", C.c_uint16), ("rows", C.c_uint16),
                ("pitch", C.c_uint32), ("offset", C.c_uint32)]


class CFont(C.Structure):  # asciichat_raster_font_t
    _fields_ = [("cell_w", C.c_int32), ("cell_h", C.c_int32), ("baseline", C.c_int32), ("n_glyphs", C.c_int32),
                ("glyphs", C.POINTER(CGlyph)), ("coverage", C.c_void_p), ("coverage_bytes", C.c_size_t),
                ("default_fg", C.c_uint32), ("default_bg", C.c_uint32), ("indexed", C.c_int32), ("flat_fg", C.c_uint32),
                ("flat_bg", C.c_uint32), ("matrix_map", C.c_int32)]


def c_font(font, cls=CFont, glyph_cls=CGlyph):
    """the C struct of a raster_ref.Font (it keeps its arrays alive)"""
    f = cls()
    gl = font.glyphs
    f._glyphs = (glyph_cls * max(1, len(gl)))(*[glyph_cls(g.codepoint, g.left, g.top, g.width, g.rows, g.pitch, g.offset) for g in gl])
    f._cov = np.ascontiguousarray(font.coverage, dtype=np.uint8).copy()
    f.cell_w, f.cell_h, f.baseline, f.n_glyphs = font.cell_w, font.cell_h, font.baseline, len(gl)
    f.glyphs = f._glyphs
    f.coverage, f.coverage_bytes = f._cov.ctypes.data, f._cov.size
    f.default_fg, f.default_bg, f.indexed = font.default_fg, font.default_bg, font.indexed
    f.flat_fg, f.flat_bg, f.matrix_map = font.flat_fg, font.flat_bg, int(bool(font.matrix_map))
    return f


_emu = None


def emulator():
    global _emu
    if _emu is None:
        L = C.CDLL(emubuild.shared_library("libraster_emu.so", "raster_emu_driver.cpp",
                                           ("raster_kernels.hpp", "raster.h", "asciichat_raster.h", "achip_types.h")))
        L.emu_raster_chunk.restype = C.c_int
        L.emu_raster.restype = C.c_int
        L.emu_raster.argtypes = [C.POINTER(CFont), C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
        _emu = L
    return _emu


CHUNK = 256  # RASTER_CHUNK; test_raster_emulated.py checks it against the driver's


# ---- atlases ----------------------------------------------------------------------------------------------------------------
def _atlas(cell_w, cell_h, baseline, spec, seed, **kw):
    """spec: [(codepoint, left, top, width, rows, pitch or 0, fill)], fill 'noise' | 'zero' | 'full' | an array of width * rows"""
    rng = np.random.default_rng(seed)
    glyphs, cov = [], []
    off = 3  # (no glyph at offset 0: a wrong offset shows)
    cov.append(np.full(3, 0x5A, dtype=np.uint8))
    for cp, left, top, w, rows, pitch, fill in sorted(spec, key=lambda s: s[0]):
        pitch = pitch or w
        bm = np.full((rows, pitch), 0x77, dtype=np.uint8)  # bytes between width and pitch must never show
        if isinstance(fill, str):
            body = {"noise": lambda: rng.integers(0, 256, size=(rows, w), dtype=np.uint8),
                    "zero": lambda: np.zeros((rows, w), dtype=np.uint8),
                    "full": lambda: np.full((rows, w), 255, dtype=np.uint8)}[fill]()
        else:
            body = np.asarray(fill, dtype=np.uint8).reshape(rows, w)
        bm[:, :w] = body
        glyphs.append(RR.Glyph(cp, left, top, w, rows, pitch, off))
        cov.append(bm.ravel())
        off += bm.size
    return RR.Font(cell_w, cell_h, baseline, glyphs, np.concatenate(cov), **kw)


def _build_atlases():
    a = {}
    # cell 5x7, baseline 5: y0 = 5 - top
    a["synth"] = _atlas(5, 7, 5, [
        (ord(" "), 0, 5, 5, 7, 0, "full"),      # in the atlas, never drawn
        (ord("A"), 1, 4, 3, 5, 0, "noise"),     # inside the cell
        (ord("L"), -5, 4, 7, 3, 0, "noise"),    # left = -5: the full left overhang
        (ord("R"), 2, 3, 8, 4, 0, "noise"),     # x1 = 10: the full right overhang
        (ord("U"), 0, 12, 5, 9, 0, "noise"),    # y0 = -7
        (ord("D"), 1, 2, 3, 11, 0, "noise"),    # y1 = 14
        (ord("Z"), -3, 8, 11, 13, 0, "zero"),   # all 0 but overhangs on every side: paints its bg
        (ord("P"), 0, 5, 4, 6, 9, "noise"),     # pitch > width
        (ord("B"), -5, 12, 15, 21, 0, "noise"),  # the whole allowed rectangle
        (ord("E"), 1, 4, 0, 0, 0, "noise"),     # an empty bitmap
        (0xE9, 1, 4, 3, 5, 0, "noise"),         # 2 bytes
        (0x2580, 0, 5, 5, 4, 0, "full"),        # 3 bytes: the upper half block
        (0xFFFD, 1, 5, 3, 7, 0, "noise"),
        (0x1F600, 0, 5, 5, 7, 0, "noise"),      # 4 bytes
    ], 1, default_fg=0xC8C9CA, default_bg=0x101112, flat_fg=0xCCCCCC, flat_bg=0x000000)
    a["synth_xterm"] = a["synth"].replace(indexed=RR.INDEXED_XTERM)
    a["synth_flat"] = a["synth"].replace(flat_fg=0x0A141E, flat_bg=0xF0E6DC)
    a["ramp"] = _atlas(16, 16, 12, [(ord("r"), 0, 12, 16, 16, 0, np.arange(256))], 2)
    a["matrix"] = _atlas(5, 7, 5, [(0xE900 + k, 0, 5, 5, 7, 0, "noise") for k in range(27)], 3, matrix_map=True)
    a["one"] = _atlas(1, 1, 1, [(ord("x"), 0, 1, 1, 1, 0, np.array([128])), (ord("o"), -1, 2, 3, 3, 0, "noise")], 4,
                      default_bg=0x203040)
    # two glyphs of the whole allowed rectangle of a 32x64 cell: 36 KB of coverage, beyond the LDS stage
    a["big"] = _atlas(32, 64, 48, [(ord("G"), -32, 112, 96, 192, 0, "noise"), (ord("H"), -32, 112, 96, 192, 0, "noise")], 5)
    a["none"] = RR.Font(5, 7, 5, [], np.zeros(0, dtype=np.uint8))
    # a text face for rendered frames: printable ASCII and the upper half block, cell 6x11, some glyphs a pixel over their cell
    text = [(cp, -(cp % 3 == 0), 8 + (cp % 5 == 0), 6 + (cp % 3 == 0) + (cp % 7 == 0), 9 + (cp % 4), 0, "noise") for cp in range(33, 127)]
    a["text"] = _atlas(6, 11, 8, text + [(0x2580, 0, 8, 6, 5, 0, "full")], 6, indexed=RR.INDEXED_XTERM)
    return a


ATLASES = _build_atlases()


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """frames: bytes, or None for the ACHIP_LEN_OVERFLOW sentinel.  base_off: the first image this many bytes behind a 16-byte
    boundary; pitch_extra: bytes between images; stride_extra: frame slots this much longer than a multiple of 16;
    status: the flags each frame must report (None: the restatement's)."""

    def __init__(self, atlas, cols, rows, frames, base_off=0, pitch_extra=0, stride_extra=0, status=None, l2=False):
        self.atlas, self.cols, self.rows, self.frames = atlas, cols, rows, list(frames)
        self.base_off, self.pitch_extra, self.stride_extra, self.status, self.l2 = base_off, pitch_extra, stride_extra, status, l2

    @property
    def font(self):
        return ATLASES[self.atlas]


def sgr(*p):
    return b"\x1b[" + b";".join(str(v).encode() for v in p) + b"m"


def fgc(r, g, b):
    return sgr(38, 2, r, g, b)


def bgc(r, g, b):
    return sgr(48, 2, r, g, b)


def _u(s):
    return s.encode("utf-8")


def _division_frame():
    vals = [0, 1, 2, 127, 128, 254, 255]
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(16):
        row = b""
        for _ in range(16):
            f, b = rng.choice(vals, 3), rng.choice(vals, 3)
            row += sgr(38, 2, *f, 48, 2, *b) + b"r"
        rows.append(row)
    return b"\n".join(rows)


def _overhang_frames():
    others = ["A", "P", "L", "R", "U", "D", "Z", "é", "▀"]
    out = []
    for gi, g in enumerate("LRUDZB"):
        for pos in range(9):
            rows = []
            for r in range(3):
                row = b""
                for c in range(3):
                    k = 3 * r + c
                    ch = g if k == pos else others[(k + gi + pos) % len(others)]
                    row += fgc(200 - 20 * k, 10 + 25 * k, 90 + k) + bgc(5 + 11 * k, 250 - 9 * k, 40 + 17 * k) + _u(ch)
                rows.append(row)
            out.append(b"\n".join(rows))
    # two overhangs meeting on one pixel: R from the left and L from the right over the blank middle, D from above and U from below
    out.append(fgc(255, 0, 0) + bgc(0, 0, 60) + b"R" + sgr(0) + b" " + fgc(0, 255, 0) + bgc(60, 0, 0) + b"L")
    out.append(fgc(255, 0, 0) + bgc(0, 0, 60) + b" D\n" + sgr(0) + b"\n" + fgc(0, 255, 0) + bgc(60, 0, 0) + b" U")
    out.append(b"BBB\n" + fgc(1, 2, 3) + b"BBB\n" + bgc(9, 8, 7) + b"BBB")
    return out


def _pen_frames():
    tall = fgc(250, 128, 3) + b"A\n" + b"\n" * 19 + bgc(3, 128, 250) + b"\n" + b"\n" * 17 + b"AP" + sgr(39) + b"A\n" + sgr() + b"P"
    return [
        fgc(10, 20, 30) + b"AP\n\nPA\n" + sgr(0) + b"AA",                      # used across an empty row, then a reset
        fgc(10, 20, 30) + b"A\n" + bgc(1, 2, 3) + b"\n" + b"PA" + fgc(9, 8, 7) + b"AP\nLR",  # fg and bg set in different rows; an SGR-only row
        sgr(38, 2, 100, 110, 120, 48, 2, 130, 140, 150) + b"AP\nPPP" + sgr(39) + b"A" + sgr(49) + b"P\nA",
        b"A\n" + sgr(49) + b"P\n" + sgr(39) + b"A\n" + bgc(7, 7, 7) + b"A" + sgr(0) + b"\nP",  # 39 / 49 onto an inherited pen
        b"AP" + fgc(1, 2, 3) + b"A\n" + b"P" + bgc(4, 5, 6) + b"A",            # cells before and behind a row's first SGR
        tall,
    ]


def _rep_frames():
    return [
        (b"A\x1b[5b", 0), (b"P\x1b[b", 0), (_u("▀") + b"\x1b[3b", 0), (b"A\x1b[20b", RR.OVERFLOW_COLS),
        (b"\x1b[3bA", RR.UNKNOWN), (b"A\n\x1b[2bP", RR.UNKNOWN), (fgc(1, 2, 3) + b"A" + bgc(4, 5, 6) + b"\x1b[2b", 0),
        (b"A\x1b[0b", 0), (b"AP\rA\x1b[1b", 0), (b"A\x1b[1;2b", RR.UNKNOWN), (b"A\x1b[99999999b", RR.OVERFLOW_COLS),
        (b"A\x1b[70bP", RR.OVERFLOW_COLS),
    ]


def _chunk_frames():
    out = []
    pre = fgc(9, 9, 9) + b"P\n"  # (a row in front: the row under test does not start at byte 0)
    tokens = [sgr(38, 2, 101, 102, 103) + b"A",  # 19 bytes of SGR
              _u("▀"), _u("\U0001F600"), b"A\x1b[12b"]
    for t in tokens:
        for j in range(len(t)):
            out.append(pre + b"\r" * (CHUNK - j) + t + b"P")
    for n in (CHUNK, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 1):
        body = (bgc(1, 2, 3) + b"APPA\r" + b"PAL\r") * (n // 20 + 2)
        out.append(pre + body[:n] + b"\nA")
    # a row far longer than the chunks of one pass, newlines behind it (the row starts are found in several passes)
    out.append(pre + (b"AP\r" + fgc(3, 2, 1)) * 400 + b"ZL\n" + b"A\n" * 3)
    return out


def _flag_frames():
    return [(b"A\x1b[1mA", RR.UNKNOWN), (b"\x1b[HA", RR.UNKNOWN), (b"A\x07P", RR.UNKNOWN), (b"A\xffA", RR.BAD_UTF8),
            (b"AAAAA", RR.OVERFLOW_COLS), (b"A\nA\nA", RR.OVERFLOW_ROWS), (None, RR.NO_FRAME), (b"", 0),
            (b"A\nP\n", 0), (b"A\r\nP\r\n", 0), (b"A\nP\n\n\n", 0)]


def _grammar_frames():
    """beyond the grammar's happy path: the status is the restatement's"""
    return [b"A\x1b[38;2;1;2", b"A\x1b", b"A\x1b[", b"A\xe2\x96", b"A\xe2\x96\nP", b"\xc0\x80A", b"\xed\xa0\x80A", b"\xf4\x90\x80\x80",
            b"A\x1b[31\nP", b"A\x1b[3\x1b[0mP", b"\x1b[?25lA", b"\x1b[1 qA", b"\x1b[1 2mA", b"\x1b[38;5;300mA", b"\x1b[38;2;1;2mA",
            b"\x1b[38;7mA" + sgr(48) + b"P", b"\x1b[38;2;256;0;0mA", b"\x1b[;38;5;9;mA", b"A\x1bP", b"\x7fA\x00P", b"\x80\xbfA",
            b"\x1b[31:1mA", b"A\nA\nA\n\x1b[1m\xff", b"\x1b[38;2;1;2;3;48mA", b"\xf0\x9f\x98A"]


def _indexed_frame():
    f = b""
    for lo in (30, 90):
        f += b"".join(sgr(v) + b"A" for v in range(lo, lo + 8)) + b"\n"
    for lo in (40, 100):
        f += b"".join(sgr(v) + b"P" for v in range(lo, lo + 8)) + b"\n"
    f += b"".join(sgr(38, 5, v) + b"A" for v in (0, 15, 16, 231, 232, 255)) + b"\n"
    f += b"".join(sgr(48, 5, v) + b"P" for v in (0, 15, 16, 231, 232, 255, 67, 145))
    return f


def _batch_frames():
    rng = np.random.default_rng(11)
    out = []
    for i in range(40):
        if i in (3, 17, 39):
            out.append(b"")
        elif i == 21:
            out.append(None)
        else:
            rows = []
            for _ in range(int(rng.integers(1, 5))):
                row = b""
                for _ in range(int(rng.integers(0, 9))):
                    row += fgc(*rng.integers(0, 256, 3)) + (bgc(*rng.integers(0, 256, 3)) if rng.integers(2) else b"")
                    row += _u("APLRUDZB é▀"[int(rng.integers(11))])
                rows.append(row)
            out.append(b"\n".join(rows))
    return out


def cases():
    c = {}
    c["division pin"] = Case("ramp", 16, 16, [_division_frame()])
    c["overhang 3x3"] = Case("synth", 3, 3, _overhang_frames())
    c["overhang 3x3 atlas through L2"] = Case("synth", 3, 3, _overhang_frames()[::7], l2=True)
    c["pen across rows"] = Case("synth", 5, 40, _pen_frames())
    rep = _rep_frames()
    c["rep"] = Case("synth", 8, 2, [f for f, _ in rep], status=[s for _, s in rep])
    c["chunk boundaries"] = Case("synth", 4, 3, _chunk_frames(), stride_extra=5)
    fl = _flag_frames()
    c["flags"] = Case("synth", 3, 2, [f for f, _ in fl], status=[s for _, s in fl])
    c["grammar edges"] = Case("synth", 4, 3, _grammar_frames())
    c["indexed flat"] = Case("synth_flat", 8, 6, [_indexed_frame()])
    c["indexed xterm"] = Case("synth_xterm", 8, 6, [_indexed_frame()])
    c["matrix map"] = Case("matrix", 6, 2, [b" :;~" + _u("\ue91a") + b"\n" + fgc(0, 255, 70) + b"az09" + _u("▀")], status=[0])
    geo = fgc(200, 100, 50) + b"ARL\n" + bgc(20, 40, 60) + b"UDP"
    for off in (0, 4, 8, 12):
        c[f"15 px rows base +{off}"] = Case("synth", 3, 2, [geo, geo[::-1], geo], base_off=off)
    c["15 px rows pitch +20 base +4"] = Case("synth", 3, 2, [geo, geo], base_off=4, pitch_extra=20)
    c["cell 1x1"] = Case("one", 7, 3, [b"xoxoxox\n" + fgc(255, 255, 255) + b"oooxxxo\n" + bgc(90, 0, 0) + b"x  o", b"o"], base_off=8)
    c["cell 1x1, 300 px: two tiles"] = Case("one", 300, 2, [(fgc(250, 240, 230) + b"xo") * 150 + b"\n" + b"o" * 300] * 2, base_off=12)
    c["cell 5x7, 61 cols: 305 px"] = Case("synth", 61, 2, [fgc(1, 200, 3) + b"APLRUDZB" * 7 + b"AAAAA\n" + b"B" * 61], base_off=4)
    c["cell 32x64 single cell"] = Case("big", 1, 1, [fgc(255, 128, 0) + bgc(0, 64, 128) + b"G", b"H", b" "], pitch_extra=16)
    c["cell 32x64 2x2"] = Case("big", 2, 2, [fgc(255, 128, 0) + b"GH\n" + bgc(0, 64, 128) + b"HG"])
    c["no glyphs"] = Case("none", 3, 2, [bgc(1, 2, 3) + b"AB\nC"])
    # 3 x 512 cell rows: the draw walks both tiles of a row in one workgroup; 16 resolve groups; the pen crosses 510 rows
    tall = fgc(255, 255, 255) + b"x" * 300 + b"\n" * 511 + b"o" * 299 + bgc(9, 9, 9) + b"x"
    c["cell 1x1, 300 x 512, three frames"] = Case("one", 300, 512, [tall, b"x", tall[:400]])
    c["batch of 40"] = Case("synth", 8, 4, _batch_frames(), stride_extra=3)
    return c


# ---- running a case ----------------------------------------------------------------------------------------------------------
def slab(case):
    """-> (frame bytes as one array, stride, lengths)"""
    longest = max([len(f) for f in case.frames if f is not None] + [1])
    stride = (longest + 15) // 16 * 16 + case.stride_extra
    buf = np.full(len(case.frames) * stride, 0x1B, dtype=np.uint8)  # (stale bytes behind a frame: escapes)
    lens = np.zeros(len(case.frames), dtype=np.uint32)
    for i, f in enumerate(case.frames):
        if f is None:
            lens[i] = LEN_OVERFLOW
        else:
            lens[i] = len(f)
            buf[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return buf, stride, lens


def image_bytes(case):
    f = case.font
    return 4 * case.cols * f.cell_w * case.rows * f.cell_h


def pixel_buffer(case, base=None):
    """-> (guard-filled buffer, byte index of image 0, pitch): image 0 `base_off` bytes behind a 16-byte boundary of the
    address the buffer's bytes will live at (base: a device copy's)"""
    pitch = image_bytes(case) + case.pitch_extra
    buf = np.full(64 + 16 + case.base_off + len(case.frames) * pitch + 256, FILL, dtype=np.uint8)
    start = 64 + (-((buf.ctypes.data if base is None else base) + 64)) % 16 + case.base_off
    return buf, start, pitch


_expected = {}


def expected(name, case):
    """[(image, status)] of a case's frames by the restatement, computed once"""
    if name not in _expected:
        out = []
        for f in case.frames:
            img, st = RR.render(f, case.cols, case.rows, case.font)
            img.setflags(write=False)
            out.append((img, st))
        _expected[name] = out
    return _expected[name]


def check(name, case, pixels, start, pitch, status):
    exp = expected(name, case)
    f = case.font
    H, W = case.rows * f.cell_h, case.cols * f.cell_w
    nb = 4 * W * H
    assert (pixels[:start] == FILL).all(), f"{name}: a store in front of the first image"
    for i, (img, st) in enumerate(exp):
        got = pixels[start + i * pitch:start + i * pitch + nb].reshape(H, W, 4)
        assert np.array_equal(got, img), f"{name} frame {i}: first differences (y, x, channel) {np.argwhere(got != img)[:6].tolist()}"
        assert (pixels[start + i * pitch + nb:start + (i + 1) * pitch] == FILL).all(), f"{name} frame {i}: a store beyond the image"
        assert int(status[i]) == st, f"{name} frame {i}: status {int(status[i])}, restatement {st}"
        if case.status is not None:
            assert st == case.status[i], f"{name} frame {i}: the restatement reports {st}, the case expects {case.status[i]}"
    assert (pixels[start + len(exp) * pitch:] == FILL).all(), f"{name}: a store past the last image"


def emu_run(case):
    """-> (pixels, start, pitch, status)"""
    n = len(case.frames)
    frames, stride, lens = slab(case)
    pixels, start, pitch = pixel_buffer(case)
    status = np.full(len(case.frames), 0xABABABAB, dtype=np.uint32)
    font = c_font(case.font)
    rc = emulator().emu_raster(C.byref(font), case.cols, case.rows, frames.ctypes.data, stride, lens.ctypes.data, n,
                               pixels.ctypes.data + start, pitch, status.ctypes.data, int(case.l2), None)
    assert rc == 0, "the font or the grid was refused"
    return pixels, start, pitch, status
